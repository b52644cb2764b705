// The library's exclusive int scan, out[i] = in[0] + ... + in[i - 1]: what IntScan of device_steps.h runs for every
// count-to-offset step of clean.hip, grid.hip, meshprep.hip, patch.hip, match.hip, segment.hip and pool.hip.  Three forms:
//
//   n <= 2^14           one 1024-thread block, one step                            (walk_exclusive_scan_kernel<1>)
//   2^14 < n <= 2^18    several 256-thread blocks with decoupled look-back, or -- GEOBI_SCAN_LOOKBACK=0 /
//                       geobi_set_scan_lookback(0) -- the one block walking the array in steps of 16 K
//   n > 2^18            rocPRIM (ExclusiveScan<int> of device_steps.h), the only form that needs a real temporary
//
// and the pair scan of match_coarsen's two-pass tail, two lists of n <= 2^18 in one launch (walk_exclusive_scan_kernel<2>).
// The graph levels of this path have <= ~10^5 nodes, where two rocPRIM launches (init + look-back) cost more in launch
// latency than the scan itself.
//
// Bounds.  in[i] and out[i] are touched for i < n only.  A thread owns 16 consecutive ints (block_scan.h: load_chunk /
// store_chunk); the int4 form is taken only when every pointer of the launch -- all four of the pair scan -- is 16-byte
// aligned and i0 + 16 <= n, else each int is loaded and stored on its own behind an i < n guard.  The look-back state has
// 4096 words for at most cdiv(2^18, 4096) = 64 blocks.  The wave-sum arrays have WAVES entries per list (16 for the
// walk, 4 for the look-back kernel), indexed by threadIdx.x >> 6.
#include "../../include/geobi_hip.h"

#include "block_scan.h"
#include "common.h"
#include "device_steps.h"

namespace geobi {

namespace {

constexpr int kScanEPT = 16;                      // ints per thread and step
constexpr int64_t kOneBlockScan = 1 << 14;        // up to here the one-block walk is a single step

// A/B knob with a test hook: the environment decides (unset or non-zero = on) until geobi_set_scan_lookback forces a form
Knob g_scan_lookback{"GEOBI_SCAN_LOOKBACK", 1};

// LISTS (1 or 2; in_b / out_b unused for 1) independent scans by ONE 1024-thread block walking the arrays with running
// carries.  Each thread owns 16 consecutive ints per list and step (16 K per step for the block); the loads of the next
// step are issued before the current one is scanned, the carries live in registers and the wave sums are
// double-buffered, so a step costs one barrier.
template <int LISTS>
__global__ __launch_bounds__(1024) void walk_exclusive_scan_kernel(const int* __restrict__ in_a,
                                                                   const int* __restrict__ in_b, int* __restrict__ out_a,
                                                                   int* __restrict__ out_b, int64_t n) {
  constexpr int EPT = kScanEPT, WAVES = 16, CHUNK = 64 * WAVES * EPT;
  __shared__ int wsum[2][LISTS][WAVES];
  const int* const in[2] = {in_a, in_b};
  int* const out[2] = {out_a, out_b};
  uintptr_t addr = 0;
#pragma unroll
  for (int l = 0; l < LISTS; ++l) addr |= (uintptr_t)in[l] | (uintptr_t)out[l];
  const bool vec = (addr & 15) == 0;
  const int64_t t0 = (int64_t)threadIdx.x * EPT;
  int cur[LISTS][EPT], nxt[LISTS][EPT], carry[LISTS];
#pragma unroll
  for (int l = 0; l < LISTS; ++l) {
    carry[l] = 0;
    load_chunk<EPT>(in[l], t0, n, vec, cur[l]);
  }
  int buf = 0;
  for (int64_t base = 0; base < n; base += CHUNK, buf ^= 1) {
    if (base + CHUNK < n) {
#pragma unroll
      for (int l = 0; l < LISTS; ++l) load_chunk<EPT>(in[l], base + CHUNK + t0, n, vec, nxt[l]);
    }
    int tsum[LISTS], ex[LISTS], total[LISTS];
#pragma unroll
    for (int l = 0; l < LISTS; ++l) tsum[l] = chunk_sum<EPT>(cur[l]);
    block_exclusive_scan_lists<WAVES, LISTS>(tsum, wsum[buf], ex, total);
#pragma unroll
    for (int l = 0; l < LISTS; ++l) {
      store_chunk<EPT>(out[l], base + t0, n, vec, cur[l], carry[l] + ex[l]);
      carry[l] += total[l];
#pragma unroll
      for (int q = 0; q < EPT; ++q) cur[l][q] = nxt[l][q];
    }
  }
}

// Exclusive scan of 16 K .. 256 K ints in ONE launch of several blocks (decoupled look-back): the one-block walk above
// is bound by a single CU's memory throughput.  Blocks take their index from a ticket (so every predecessor of a block is
// already running: the look-back cannot wait on a block that has not started), publish (epoch | flag | value) as one
// 64-bit word -- flag 1: the block's own sum, flag 2: the inclusive prefix up to and including it -- and wave 0 of each
// block inspects 64 predecessors at a time.  The state words carry the call's epoch, so the buffer is never cleared
// between calls.
__device__ __forceinline__ unsigned long long scan_pack(unsigned epoch, unsigned flag, int value) {
  return ((unsigned long long)((epoch << 2) | flag) << 32) | (unsigned)value;
}

__global__ __launch_bounds__(256) void lookback_exclusive_scan_kernel(const int* __restrict__ in, int* __restrict__ out,
                                                                      int64_t n, unsigned long long* state, int* ticket,
                                                                      unsigned epoch, int nblocks) {
  constexpr int EPT = kScanEPT, WAVES = 4, CHUNK = 64 * WAVES * EPT;
  __shared__ int s_bid, s_prefix, wsum[WAVES];
  if (threadIdx.x == 0) s_bid = atomicAdd(ticket, 1);
  __syncthreads();
  const int b = s_bid;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)b * CHUNK + (int64_t)threadIdx.x * EPT;
  const bool vec = ((((uintptr_t)in) | ((uintptr_t)out)) & 15) == 0;
  int v[EPT];
  load_chunk<EPT>(in, i0, n, vec, v);
  int total;
  const int ex = block_exclusive_scan<WAVES, false>(chunk_sum<EPT>(v), wsum, total);   // wsum: written once per block
  if (wave == 0) {
    int prefix = 0;
    if (b > 0) {
      if (lane == 0) __hip_atomic_store(state + b, scan_pack(epoch, 1, total), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      for (int hi = b - 1; hi >= 0; hi -= 64) {
        const int pidx = hi - lane;
        unsigned flag = 2;
        int val = 0;
        if (pidx >= 0) {
          unsigned long long st;
          int spins = 0;
          do {
            st = __hip_atomic_load(state + pidx, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
          } while (((unsigned)(st >> 34) != epoch || ((st >> 32) & 3) == 0) && ++spins < (1 << 26));
          flag = (unsigned)(st >> 32) & 3;
          val = (int)(unsigned)st;
        }
        const unsigned long long done = __ballot(flag == 2);
        const int first = done ? __ffsll((long long)done) - 1 : 64;       // nearest predecessor with a full prefix
        int c = lane <= first ? val : 0;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
        prefix += c;
        if (done) break;
      }
    }
    if (lane == 0) {
      __hip_atomic_store(state + b, scan_pack(epoch, 2, prefix + total), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      s_prefix = prefix;
      if (b == nblocks - 1) *ticket = 0;                                   // every ticket of this call is taken
    }
  }
  __syncthreads();
  store_chunk<EPT>(out, i0, n, vec, v, s_prefix + ex);
}

// persistent look-back state (zeroed once; see the kernel).  One per host thread: a thread drives one stream at a time
// (one mesh group of a concurrent step, executor.hip), so two scans in flight never share state words.
thread_local unsigned long long* g_scan_state = nullptr;
thread_local int* g_scan_ticket = nullptr;
thread_local unsigned g_scan_epoch = 0;
constexpr size_t kScanStateBytes = 4096 * sizeof(unsigned long long);

hipError_t lookback_scan(const int* in, int* out, int64_t n, hipStream_t s) {
  if (g_scan_state == nullptr) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, kScanStateBytes + 256);
    if (e != hipSuccess) return e;
    // zeroed ON THE LAUNCH STREAM: a null-stream memset is not ordered against a non-blocking stream, and a host thread
    // that starts later (one context per thread) initialises its state while other threads' kernels are in flight
    e = hipMemsetAsync(p, 0, kScanStateBytes + 256, s);
    if (e != hipSuccess) return e;
    g_scan_state = (unsigned long long*)p;
    g_scan_ticket = (int*)((char*)p + kScanStateBytes);
  }
  g_scan_epoch = (g_scan_epoch + 1) & 0x3fffffffu;
  if (g_scan_epoch == 0) g_scan_epoch = 1;
  const int nblocks = cdiv(n, 4096);
  lookback_exclusive_scan_kernel<<<nblocks, 256, 0, s>>>(in, out, n, g_scan_state, g_scan_ticket, g_scan_epoch, nblocks);
  return hipGetLastError();
}

}  // namespace

size_t scan_ws_bytes(int64_t n) { return n <= kSmallScan ? 16 : ExclusiveScan<int>::temp_bytes(n); }

int scan_exclusive_i32(void* temp, size_t temp_bytes, const int* in, int* out, int64_t n, hipStream_t s) {
  hipError_t e;
  if (n > kSmallScan) {
    prof_begin(PROF_POOL_FORM, s, 0.0, POOL_FORM_SCAN_ROCPRIM);
    e = ExclusiveScan<int>::call(const_cast<int*>(in), out, n, s)(temp, temp_bytes);
  } else if (g_scan_lookback.on() && n > kOneBlockScan) {
    prof_begin(PROF_POOL_FORM, s, 0.0, POOL_FORM_SCAN_LOOKBACK);
    e = lookback_scan(in, out, n, s);
  } else {
    prof_begin(PROF_POOL_FORM, s, 0.0, POOL_FORM_SCAN_ONE_BLOCK);
    walk_exclusive_scan_kernel<1><<<1, 1024, 0, s>>>(in, nullptr, out, nullptr, n);
    e = hipGetLastError();
  }
  prof_end(PROF_POOL_FORM, s);
  GEOBI_HIP(e);
  return 0;
}

// n <= kSmallScan is the caller's test (match_coarsen, the debug entry): above it two IntScan runs are the faster form
int scan_exclusive_i32_pair(const int* in_a, const int* in_b, int* out_a, int* out_b, int64_t n, hipStream_t s) {
  if (n <= 0) return 0;
  walk_exclusive_scan_kernel<2><<<1, 1024, 0, s>>>(in_a, in_b, out_a, out_b, n);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // namespace geobi

using namespace geobi;

extern "C" {

// Test hook: 1 / 0 force the look-back form, a negative value goes back to what the environment says.
int geobi_set_scan_lookback(int on) {
  if (on < 0) g_scan_lookback.reset(); else g_scan_lookback.set(on != 0);
  return 0;
}

size_t geobi_debug_scan_ws_bytes(int64_t n) { return scan_ws_bytes(n); }
int geobi_debug_scan_exclusive_i32(const int32_t* in, int32_t* out, int64_t n, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(0, n);
  if (n <= 0) return 0;
  GEOBI_NOTNULL(in); GEOBI_NOTNULL(out); GEOBI_NOTNULL(ws);
  GEOBI_REQUIRE(ws_bytes >= scan_ws_bytes(n), "%s: workspace too small (%zu < %zu)", __func__, ws_bytes, scan_ws_bytes(n));
  return scan_exclusive_i32(ws, ws_bytes, in, out, n, as_stream(stream));
}
int geobi_debug_scan_exclusive_i32_pair(const int32_t* in_a, const int32_t* in_b, int32_t* out_a, int32_t* out_b, int64_t n,
                                        void* stream) {
  GEOBI_SIZES(0, n);
  if (n <= 0) return 0;
  GEOBI_NOTNULL(in_a); GEOBI_NOTNULL(in_b); GEOBI_NOTNULL(out_a); GEOBI_NOTNULL(out_b);
  GEOBI_REQUIRE(n <= kSmallScan, "%s: n = %lld, the pair scan takes at most 2^18 elements", __func__, (long long)n);
  return scan_exclusive_i32_pair(in_a, in_b, out_a, out_b, n, as_stream(stream));
}

}  // extern "C"
