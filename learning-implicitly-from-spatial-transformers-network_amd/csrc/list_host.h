// Host-side plumbing shared by the translation units of the C ABI (list_capi.hip and the *_kernels.hip files that
// export a section of their own).  Not part of the C ABI.
//
// Everything here is static: each unit that includes this header gets its OWN thread-local error text, the
// one its list_*_last_error() returns -- a failing Chamfer call leaves list_mesh_last_error() as it was.
#pragma once

#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <hip/hip_runtime.h>

#include "list_hip.h"

static thread_local char g_err[512] = "";

// Sets this unit's error text and returns `code`: `return fail(LIST_ERR_ARG, "x is NULL");`
__attribute__((format(printf, 2, 3))) static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

static int hip_fail(hipError_t e, const char* what) { return fail(LIST_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); }

// After a kernel launch: LIST_OK, or the launch error under the kernel's name
static int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? LIST_OK : hip_fail(e, what);
}

// Refusal of a workspace smaller than `sizing_fn` (the section's list_*_workspace_bytes) asks for
static int workspace_too_small(size_t have, size_t need, const char* sizing_fn) {
  return fail(LIST_ERR_WORKSPACE, "workspace %zu bytes, need %zu (%s)", have, need, sizing_fn);
}

// Refusal of a packed-weights blob smaller than the section's list_*_weight_bytes asks for
static int packed_too_small(const char* what, size_t have, size_t need) {
  return fail(LIST_ERR_WORKSPACE, "%s: packed holds %zu bytes, need %zu", what, have, need);
}

// LIST_OK when [begin, end) is a range of the n launches of a list_*_forward_steps (`what`), else its refusal
static int check_step_range(const char* what, int32_t begin, int32_t end, int32_t n) {
  if (begin < 0 || end > n || begin > end)
    return fail(LIST_ERR_ARG, "%s: steps [%d, %d) outside [0, %d]", what, begin, end, n);
  return LIST_OK;
}

static bool misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }      // a: a power of two

static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }      // workspace regions start on 256 bytes

static int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Workgroups of `threads` that cover n items, and the same clamped to [1, cap] (for kernels that stride over the grid)
static unsigned blocks_for(int64_t n, int threads) { return (unsigned)cdiv(n, threads); }
static unsigned blocks_capped(int64_t n, int threads, int64_t cap) {
  const int64_t b = cdiv(n, threads);
  return (unsigned)(b < 1 ? 1 : b < cap ? b : cap);
}

// Carves "region a | region b | ... " out of a workspace or a packed blob: take(bytes) is where the region starts, and
// the next one starts align_up(bytes) later.  Every region so starts on 256 bytes, which is why advancing by
// `o += align_up(bytes)` and by `o = align_up(o + bytes)` give the same offsets: for o a multiple of 256 the two are equal.
struct Carver {
  size_t next = 0;
  size_t take(size_t bytes) { const size_t at = next; next += align_up(bytes); return at; }
  size_t total() const { return next; }
};

// The region at byte offset `off` of a workspace, as T
template <typename T> static T* at(void* ws, size_t off) { return (T*)((char*)ws + off); }
template <typename T> static const T* at(const void* ws, size_t off) { return (const T*)((const char*)ws + off); }

// Launches `kernel` (no dynamic LDS: no stage uses any) and returns launched(name):
//   if (int rc = launch("mc_count_kernel", mc_count_kernel, grid, block, s, volume, X, ...)) return rc;
template <typename K, typename... Args>
static int launch(const char* name, K kernel, dim3 grid, dim3 block, hipStream_t stream, Args... args) {
  hipLaunchKernelGGL(kernel, grid, block, 0, stream, args...);
  return launched(name);
}
