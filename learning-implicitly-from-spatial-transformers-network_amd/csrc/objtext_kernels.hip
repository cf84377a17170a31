// The text of a Wavefront .obj file composed on the device (include/list_objtext.h; the rule itself is
// csrc/objtext_math.h).  Line i of the file is vertex i for i < V and face i - V after that; N = V + F.
//
//   k_objtext_len        one lane per line: its byte length (int64); entry N is 0, so that the scan's entry N is the
//                        file's length and its entry V the length of the vertex lines.
//   hipCUB exclusive scan over the N + 1 lengths: every line's byte offset.
//   k_objtext_totals     one lane copies those two entries into the caller's totals.
//   k_objtext_emit       a workgroup takes kLines consecutive lines, one per lane: one contiguous span of the output of
//                        at most kLines * 74 bytes.  Each lane formats its line again (the digits are recomputed, not
//                        kept: DESIGN section 24) and puts its bytes into LDS at the line's place in the span, the span
//                        shifted by the low four bits of its first byte's address, so that LDS byte j and global byte
//                        base + j are aligned alike.  After one barrier the workgroup writes the span out in 16-byte
//                        pieces: a piece that lies wholly inside the span is one aligned 16-byte store, the span's
//                        unaligned head and tail pieces are written byte by byte, and only the bytes that are the
//                        span's and lie below n_out_bytes.
//
// Nothing here waits for another thread beyond that barrier; there are no atomics.
#include <hip/hip_runtime.h>

#include "list_objtext.h"
#include "list_cub.h"
#include "list_host.h"
#include "objtext_math.h"

namespace {

constexpr int kLines = 256;                                         // lines, and threads, per workgroup
constexpr int kSpanBytes = kLines * OBJTEXT_MAX_VERTEX_LINE;        // the longest span
constexpr int kStageBytes = kSpanBytes + 16;                        // ... shifted by up to 15 bytes, a multiple of 16

static_assert(OBJTEXT_MAX_FACE_LINE <= OBJTEXT_MAX_VERTEX_LINE && kStageBytes % 16 == 0, "the stage holds any span");
static_assert(LIST_OBJTEXT_MAX_TOKEN == OBJTEXT_MAX_TOKEN && LIST_OBJTEXT_MAX_VERTEX_LINE == OBJTEXT_MAX_VERTEX_LINE &&
                  LIST_OBJTEXT_MAX_FACE_LINE == OBJTEXT_MAX_FACE_LINE,
              "list_objtext.h and objtext_math.h state the same bounds");

struct LdsSink {
  uint8_t* p;
  __device__ __forceinline__ void put(uint8_t c) { *p++ = c; }
};

__device__ __forceinline__ void load3(const void* base, int64_t row, uint32_t w[3]) {
  const uint32_t* p = (const uint32_t*)base + 3 * row;
  w[0] = p[0], w[1] = p[1], w[2] = p[2];
}

__global__ __launch_bounds__(kLines) void k_objtext_len(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                        int64_t V, int64_t N, int64_t* __restrict__ len) {
  const int64_t i = (int64_t)blockIdx.x * kLines + threadIdx.x;
  if (i > N) return;
  int32_t n = 0;
  uint32_t w[3];
  if (i < V) {
    load3(verts, i, w);
    n = objtext_vertex_len(w);
  } else if (i < N) {
    load3(faces, i - V, w);
    const int32_t f[3] = {(int32_t)w[0], (int32_t)w[1], (int32_t)w[2]};
    n = objtext_face_len(f);
  }
  len[i] = n;
}

__global__ void k_objtext_totals(const int64_t* __restrict__ off, int64_t V, int64_t N, int64_t* __restrict__ totals) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    totals[0] = off[N];
    totals[1] = off[V];
  }
}

__global__ __launch_bounds__(kLines) void k_objtext_emit(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                         int64_t V, int64_t N, const int64_t* __restrict__ off,
                                                         uint8_t* __restrict__ out, int64_t n_out) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
  const int64_t first = (int64_t)blockIdx.x * kLines;               // < N: the grid covers the lines exactly
  const int64_t last = first + kLines < N ? first + kLines : N;
  const int64_t span0 = off[first], span1 = off[last];
  if (span0 >= n_out) return;                                       // the whole workgroup: nothing of this span is wanted
  const int pad = (int)(((uintptr_t)out + (uint64_t)span0) & 15u);

  const int64_t i = first + threadIdx.x;
  if (i < N) {
    const int64_t rel = off[i] - span0;
    // offsets this call did not compute (a workspace touched in between) must not become LDS addresses
    if (rel >= 0 && rel <= kSpanBytes - OBJTEXT_MAX_VERTEX_LINE) {
      LdsSink sink = {stage + pad + (int)rel};
      uint32_t w[3];
      if (i < V) {
        load3(verts, i, w);
        objtext_vertex_put(w, sink);
      } else {
        load3(faces, i - V, w);
        const int32_t f[3] = {(int32_t)w[0], (int32_t)w[1], (int32_t)w[2]};
        objtext_face_put(f, sink);
      }
    }
  }
  __syncthreads();

  int64_t want = (span1 < n_out ? span1 : n_out) - span0;           // bytes of this span to write
  want = want < 0 ? 0 : want > kSpanBytes ? kSpanBytes : want;
  const int end = pad + (int)want;                                  // the span is stage[pad, end)
  uint8_t* base = out + span0 - pad;                                // 16-byte aligned; base + j is stage[j]'s place
  for (int lo = 16 * (int)threadIdx.x; lo < end; lo += 16 * kLines) {
    if (lo >= pad && lo + 16 <= end) {
      *(uint4*)(base + lo) = *(const uint4*)(stage + lo);
    } else {                                                        // the head or the tail piece
      const int a = lo > pad ? lo : pad, b = lo + 16 < end ? lo + 16 : end;
      for (int j = a; j < b; ++j) base[j] = stage[j];
    }
  }
}

struct Layout {
  size_t len, off, scratch, scratch_bytes, total;
};

int check_sizes(int64_t V, int64_t F) {
  if (V < 0 || F < 0 || V >= INT32_MAX || F >= INT32_MAX || V + F >= INT32_MAX)
    return fail(LIST_ERR_SHAPE, "V = %lld, F = %lld: need 0 <= V, F and V + F < INT32_MAX", (long long)V, (long long)F);
  return LIST_OK;
}

// the layout, or false with the refusal's message set
bool layout(int64_t N, Layout* L) {
  if (!exclusive_sum_scratch<int64_t>(N + 1, &L->scratch_bytes)) return false;
  Carver c;
  L->len = c.take((size_t)(N + 1) * sizeof(int64_t));
  L->off = c.take((size_t)(N + 1) * sizeof(int64_t));
  L->scratch = c.take(L->scratch_bytes);
  L->total = c.total();
  return true;
}

int check_call(const float* verts, const int32_t* faces, int64_t V, int64_t F, const void* workspace,
               size_t workspace_bytes, Layout* L) {
  if (int rc = check_sizes(V, F)) return rc;
  if (!workspace || (V && !verts) || (F && !faces)) return fail(LIST_ERR_ARG, "verts/faces/workspace is NULL");
  if (!layout(V + F, L)) return LIST_ERR_HIP;       // checked last: the size comes from hipCUB, which asks the device
  if (workspace_bytes < L->total) return workspace_too_small(workspace_bytes, L->total, "list_objtext_workspace_bytes");
  return LIST_OK;
}

}  // namespace

extern "C" {

const char* list_objtext_last_error(void) { return g_err; }

size_t list_objtext_workspace_bytes(int64_t V, int64_t F) {
  Layout L;
  return check_sizes(V, F) == LIST_OK && layout(V + F, &L) ? L.total : 0;
}

int list_objtext_count(const float* verts, const int32_t* faces, int64_t V, int64_t F, void* workspace,
                       size_t workspace_bytes, int64_t* totals, void* stream) {
  Layout L;
  if (int rc = check_call(verts, faces, V, F, workspace, workspace_bytes, &L)) return rc;
  if (!totals) return fail(LIST_ERR_ARG, "totals is NULL");
  hipStream_t s = (hipStream_t)stream;
  const int64_t N = V + F;
  int64_t *len = at<int64_t>(workspace, L.len), *off = at<int64_t>(workspace, L.off);
  if (int rc = launch("k_objtext_len", k_objtext_len, dim3(blocks_for(N + 1, kLines)), dim3(kLines), s, verts, faces, V,
                      N, len))
    return rc;
  if (int rc = exclusive_sum(at<char>(workspace, L.scratch), L.scratch_bytes, (const int64_t*)len, off, N + 1, s)) return rc;
  return launch("k_objtext_totals", k_objtext_totals, dim3(1), dim3(64), s, (const int64_t*)off, V, N, totals);
}

int list_objtext_emit(const float* verts, const int32_t* faces, int64_t V, int64_t F, const void* workspace,
                      size_t workspace_bytes, uint8_t* out, int64_t n_out_bytes, void* stream) {
  Layout L;
  if (int rc = check_call(verts, faces, V, F, workspace, workspace_bytes, &L)) return rc;
  if (n_out_bytes < 0 || (n_out_bytes && !out))
    return fail(LIST_ERR_ARG, "n_out_bytes = %lld, out %s", (long long)n_out_bytes, out ? "given" : "NULL");
  const int64_t N = V + F;
  if (N == 0 || n_out_bytes == 0) return LIST_OK;
  return launch("k_objtext_emit", k_objtext_emit, dim3(blocks_for(N, kLines)), dim3(kLines), (hipStream_t)stream, verts,
                faces, V, N, at<int64_t>(workspace, L.off), out, n_out_bytes);
}

int64_t list_objtext_host(const float* verts, const int32_t* faces, int64_t V, int64_t F, uint8_t* out, int64_t cap) {
  if (V < 0 || F < 0 || cap < 0) return fail(LIST_ERR_SHAPE, "V = %lld, F = %lld, cap = %lld: none may be negative",
                                             (long long)V, (long long)F, (long long)cap);
  if ((V && !verts) || (F && !faces) || (cap && !out)) return fail(LIST_ERR_ARG, "verts/faces/out is NULL");
  return objtext_host_file(verts, faces, V, F, out, cap);
}

}  // extern "C"
