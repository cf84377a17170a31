// hipCUB's two-phase calls, shared by the units that scan or sort (mesh, refine, components, eval, simplify, objtext): the scratch size
// query that a layout makes, and the run on the carved scratch region.  Not part of the C ABI.
//
// A query returns false with the unit's error text set (LIST_ERR_HIP); a run returns LIST_OK or the HIP error under
// the call's name.  The scans take their input as the call site has it (In: T* or const T*): hipCUB instantiates its
// kernels per iterator type.
#pragma once

#include <hipcub/hipcub.hpp>

#include "list_host.h"

static bool cub_sized(hipError_t e, const char* call) {
  if (e != hipSuccess) fail(LIST_ERR_HIP, "%s: scratch size query failed", call);
  return e == hipSuccess;
}

static int cub_ran(hipError_t e, const char* call) { return e == hipSuccess ? LIST_OK : hip_fail(e, call); }

template <typename T> static bool exclusive_sum_scratch(int64_t n, size_t* bytes) {
  *bytes = 0;
  return cub_sized(hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (const T*)nullptr, (T*)nullptr, (int)n),
                   "hipcub::DeviceScan::ExclusiveSum");
}

template <typename In, typename T>
static int exclusive_sum(void* scratch, size_t scratch_bytes, In in, T* out, int64_t n, hipStream_t s) {
  return cub_ran(hipcub::DeviceScan::ExclusiveSum(scratch, scratch_bytes, in, out, (int)n, s),
                 "hipcub::DeviceScan::ExclusiveSum");
}

template <typename T> static bool inclusive_sum_scratch(int64_t n, size_t* bytes) {
  *bytes = 0;
  return cub_sized(hipcub::DeviceScan::InclusiveSum(nullptr, *bytes, (const T*)nullptr, (T*)nullptr, (int)n),
                   "hipcub::DeviceScan::InclusiveSum");
}

template <typename In, typename T>
static int inclusive_sum(void* scratch, size_t scratch_bytes, In in, T* out, int64_t n, hipStream_t s) {
  return cub_ran(hipcub::DeviceScan::InclusiveSum(scratch, scratch_bytes, in, out, (int)n, s),
                 "hipcub::DeviceScan::InclusiveSum");
}

// Pairs sorted by bits [0, end_bit) of their keys
template <typename K, typename V> static bool sort_pairs_scratch(int64_t n, int end_bit, size_t* bytes) {
  *bytes = 0;
  return cub_sized(hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, (const K*)nullptr, (K*)nullptr, (const V*)nullptr,
                                                      (V*)nullptr, (int)n, 0, end_bit),
                   "hipcub::DeviceRadixSort::SortPairs");
}

template <typename K, typename V>
static int sort_pairs(void* scratch, size_t scratch_bytes, const K* keys_in, K* keys_out, const V* vals_in, V* vals_out,
                      int64_t n, int end_bit, hipStream_t s) {
  return cub_ran(hipcub::DeviceRadixSort::SortPairs(scratch, scratch_bytes, keys_in, keys_out, vals_in, vals_out, (int)n,
                                                    0, end_bit, s),
                 "hipcub::DeviceRadixSort::SortPairs");
}
