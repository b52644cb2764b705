// Temporary-storage sizes of the rocPRIM calls of graph.hip, pool.hip, sample.hip and the mesh tools (through
// edge_table.h), for Arena::take_ws.  Kept out of common.h: only these units compile rocPRIM.
// 0: the size query failed (it asks the device for its properties, so it fails on a host without one); take_ws then
// fails the carve and the enclosing *_ws_bytes answers 0.  A query that succeeds answers at least 16.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace geobi {

static inline size_t temp_bytes_or_0(hipError_t e, size_t tb) { return e != hipSuccess ? 0 : (tb > 16 ? tb : 16); }

// radix sort of n (K, V) pairs / of n keys K over the key bits 0 .. bits
template <typename K, typename V>
static inline size_t sort_pairs_temp_bytes(int64_t n, unsigned bits = 8 * sizeof(K)) {
  size_t tb = 0;
  if (n <= 0) return 16;
  return temp_bytes_or_0(rocprim::radix_sort_pairs(nullptr, tb, (K*)nullptr, (K*)nullptr, (V*)nullptr, (V*)nullptr,
                                                   (size_t)n, 0u, bits, (hipStream_t)0, false), tb);
}
template <typename K>
static inline size_t sort_keys_temp_bytes(int64_t n, unsigned bits = 8 * sizeof(K)) {
  size_t tb = 0;
  if (n <= 0) return 16;
  return temp_bytes_or_0(rocprim::radix_sort_keys(nullptr, tb, (K*)nullptr, (K*)nullptr, (size_t)n, 0u, bits,
                                                  (hipStream_t)0, false), tb);
}
// exclusive plus-scan of n values T
template <typename T>
static inline size_t scan_temp_bytes(int64_t n) {
  size_t tb = 0;
  return temp_bytes_or_0(rocprim::exclusive_scan(nullptr, tb, (T*)nullptr, (T*)nullptr, (T)0, (size_t)n,
                                                 rocprim::plus<T>(), (hipStream_t)0, false), tb);
}
// inclusive plus-scan of n values T
template <typename T>
static inline size_t inclusive_scan_temp_bytes(int64_t n) {
  size_t tb = 0;
  return temp_bytes_or_0(rocprim::inclusive_scan(nullptr, tb, (T*)nullptr, (T*)nullptr, (size_t)n, rocprim::plus<T>(),
                                                 (hipStream_t)0, false), tb);
}

}  // namespace geobi
