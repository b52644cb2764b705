// Device sorts and scans as step records, host-only, and the one header that compiles rocPRIM.  A record is
// taken from the Arena in a unit's carve -- one take_ws, sized by the primitive's own query for the record's types, count
// and key bits -- and is then the only way to run the step.  It owns no data buffers, and one temporary may serve several
// runs on a stream.  A run may be shorter or sort fewer bits than the take; more is refused by name before anything is
// enqueued.  Inputs are not written, but are plain pointers: a run then launches the kernel instances the query names.
#pragma once
#include "common.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace geobi {

// A record's call(...) binds the arguments of its rocPRIM call and leaves (temp, bytes) open, for the size query and the run.
// A query that fails (it asks the device for its properties) answers 0, which fails the carve; one that succeeds, >= 16.
template <typename Call>
static inline size_t query_bytes(Call&& call) {
  size_t tb = 0;
  return call(nullptr, tb) != hipSuccess ? 0 : (tb > 16 ? tb : 16);
}
template <typename Call>
static inline int run_step(const char* step, SubWs temp, int64_t n_run, int64_t n, unsigned bits_run, unsigned bits, Call&& call) {
  GEOBI_REQUIRE(n_run <= n && bits_run <= bits, "%s: a run of %lld elements, %u key bits, does not fit its take of %lld, %u",
                step, (long long)n_run, bits_run, (long long)n, bits);
  GEOBI_HIP(call(temp.p, temp.bytes));
  return 0;
}

// ---- stable radix sort of n (K, V) pairs over the key bits 0 .. bits
template <typename K, typename V>
struct PairSort {
  SubWs temp; int64_t n; unsigned bits;
  static auto call(K* k_in, K* k_out, V* v_in, V* v_out, int64_t n, unsigned bits, hipStream_t s) {
    return [=](void* t, size_t& tb) { return rocprim::radix_sort_pairs(t, tb, k_in, k_out, v_in, v_out, (size_t)n, 0u, bits, s, false); };
  }
  static PairSort take(Arena& a, int64_t n, unsigned bits = 8 * sizeof(K)) {
    return {a.take_ws(n <= 0 ? 16 : query_bytes(call(0, 0, 0, 0, n, bits, 0))), n, bits};
  }
  // what a run of n_run pairs wants, for the unit whose take is no bound of it by construction (grid.hip)
  int need(int64_t n_run, size_t* bytes) const { *bytes = 0; GEOBI_HIP(call(0, 0, 0, 0, n_run, bits, 0)(nullptr, *bytes)); return 0; }
  int run(K* k_in, K* k_out, V* v_in, V* v_out, int64_t n_run, unsigned bits_run, hipStream_t s) const {
    return run_step("PairSort", temp, n_run, n, bits_run, bits, call(k_in, k_out, v_in, v_out, n_run, bits_run, s));
  }
  int run(K* k_in, K* k_out, V* v_in, V* v_out, hipStream_t s) const { return run(k_in, k_out, v_in, v_out, n, bits, s); }
};

// ---- radix sort of n keys K over the key bits 0 .. bits
template <typename K>
struct KeySort {
  SubWs temp; int64_t n; unsigned bits;
  static auto call(K* k_in, K* k_out, int64_t n, unsigned bits, hipStream_t s) {
    return [=](void* t, size_t& tb) { return rocprim::radix_sort_keys(t, tb, k_in, k_out, (size_t)n, 0u, bits, s, false); };
  }
  static KeySort take(Arena& a, int64_t n, unsigned bits = 8 * sizeof(K)) {
    return {a.take_ws(n <= 0 ? 16 : query_bytes(call(0, 0, n, bits, 0))), n, bits};
  }
  int run(K* k_in, K* k_out, int64_t n_run, unsigned bits_run, hipStream_t s) const {
    return run_step("KeySort", temp, n_run, n, bits_run, bits, call(k_in, k_out, n_run, bits_run, s));
  }
  int run(K* k_in, K* k_out, hipStream_t s) const { return run(k_in, k_out, n, bits, s); }
};

// ---- rocPRIM's plus-scan of n values T from 0, exclusive or inclusive
template <typename T, bool kInclusive>
struct PrimScan {
  SubWs temp; int64_t n;
  static auto call(T* in, T* out, int64_t n, hipStream_t s) {
    return [=](void* t, size_t& tb) {
      if constexpr (kInclusive) return rocprim::inclusive_scan(t, tb, in, out, (size_t)n, rocprim::plus<T>(), s, false);
      else return rocprim::exclusive_scan(t, tb, in, out, (T)0, (size_t)n, rocprim::plus<T>(), s, false);
    };
  }
  static size_t temp_bytes(int64_t n) { return query_bytes(call(0, 0, n, 0)); }
  static PrimScan take(Arena& a, int64_t n) { return {a.take_ws(temp_bytes(n)), n}; }
  int run(T* in, T* out, int64_t n_run, hipStream_t s) const { return run_step("PrimScan", temp, n_run, n, 0, 0, call(in, out, n_run, s)); }
  int run(T* in, T* out, hipStream_t s) const { return run(in, out, n, s); }
};
template <typename T> using ExclusiveScan = PrimScan<T, false>;
template <typename T> using InclusiveScan = PrimScan<T, true>;

// ---- the library's own exclusive int scan (scan.hip): one block up to 2^14 elements, the look-back kernel up to 2^18,
// rocPRIM (ExclusiveScan<int>'s call and size) above.  Not ExclusiveScan<int>: below 2^18 elements another kernel runs
// and the temporary is 16 bytes.
struct IntScan {
  SubWs temp; int64_t n;
  int run(const int* in, int* out, int64_t n_run, hipStream_t s) const {
    GEOBI_REQUIRE(n_run <= n, "IntScan: a run of %lld elements does not fit its take of %lld", (long long)n_run, (long long)n);
    return scan_exclusive_i32(temp.p, temp.bytes, in, out, n_run, s);
  }
  int run(const int* in, int* out, hipStream_t s) const { return run(in, out, n, s); }
  static IntScan take(Arena& a, int64_t n) { return {a.take_ws(scan_ws_bytes(n)), n}; }
};

// ---- n counts (or flags) and the scan over them: the count-to-offset step of match.hip, segment.hip and pool.hip
struct CountScan { int* cnt; IntScan scan; };
static inline CountScan carve_count_scan(Arena& a, int64_t n) { return {a.take<int>(n), IntScan::take(a, n)}; }

// ---- 64-bit sort keys (a << bits) | b of graph.hip, segment.hip and pool.hip, with (1 << bits) > N: the radix sort only
// has to look at 2 * bits bits (34 for the 82 k-node level-0 facet graph) instead of 64.  The sentinel (all ones) still
// sorts last because every valid key is < 2^(2 bits) - 1.
constexpr uint64_t kSentinel = ~0ull;
static inline int key_bits(int64_t N) {
  int b = 1;
  while ((1ll << b) <= N) ++b;
  return b;
}

}  // namespace geobi
