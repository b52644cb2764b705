// The coarse graph's edges, the back half of a pooling step (pool_edge, the reference's net_util.py:289-295), with their
// entry points: relabel the endpoints by the clustering, drop loops, merge duplicates by mean.  match.hip finds the
// clustering, segment.hip holds the member lists these builders read.
//
//   pool_edge         any clustering: one radix sort of the relabelled edges (PairSort)
//   pool_edge_rows    a matching: one wave per coarse node sorts the <= 64 entries of its members' rows in registers --
//                     two passes around a scan, or the one-pass form that parks the rows and compacts them after it
//
// The count-to-offset scans are CountScan records (device_steps.h).
#include "../../include/geobi_hip.h"

#include "common.h"
#include "device_steps.h"

namespace geobi {

namespace {

// ---------------------------------------------------------------------------- pool_edge
__global__ void pool_edge_keys_kernel(const int* __restrict__ cnew, const int* __restrict__ row,
                                      const int* __restrict__ col, int64_t E, int bits,
                                      uint64_t* __restrict__ keys, int* __restrict__ vals) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  int a = cnew[row[e]], b = cnew[col[e]];
  keys[e] = (a == b) ? kSentinel : (((uint64_t)(uint32_t)a << bits) | (uint64_t)(uint32_t)b);
  vals[e] = (int)e;
}

__global__ void pool_edge_heads_kernel(const uint64_t* __restrict__ keys, int64_t E, int* __restrict__ head) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  uint64_t k = keys[e];
  head[e] = (k != kSentinel && (e == 0 || keys[e - 1] != k)) ? 1 : 0;
}

__global__ void pool_edge_emit_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ vals,
                                      const int* __restrict__ head, const int* __restrict__ rank,
                                      const float* __restrict__ w, int64_t E, int* __restrict__ row_c,
                                      int* __restrict__ col_c, float* __restrict__ w_c, uint64_t* __restrict__ ukeys,
                                      int* __restrict__ count, int bits) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  if (e == E - 1) *count = rank[e] + head[e];
  if (!head[e]) return;
  uint64_t k = keys[e];
  int o = rank[e];
  row_c[o] = (int)(uint32_t)(k >> bits);
  col_c[o] = (int)(uint32_t)(k & ((1ull << bits) - 1));
  ukeys[o] = k;
  if (w) {
    // mean of the merged duplicates; fp64 accumulation makes the result independent of the
    // order of the run, so w(a,b) == w(b,a) bit for bit and the matching stays symmetric
    double s = 0.0;
    int n = 0;
    for (int64_t f = e; f < E && keys[f] == k; ++f) { s += (double)w[vals[f]]; ++n; }
    w_c[o] = (float)(s / (double)n);
  }
}

// ---------------------------------------------------------- pool_edge, sort-free (matchings)
// For a matching every coarse node has 1-2 members, so its coarse row is the union of at most two
// fine rows: one wave per coarse node gathers those (<= 64) entries, relabels them, sorts them with a
// 64-lane bitonic network, drops the self entry and merges duplicates -- no global radix sort.
// PASS 0 counts the unique neighbours (-> exclusive scan -> rowptr), PASS 1 repeats and writes.
// Rows with more than 64 gathered entries set `overflow` (the caller falls back to the sorted path).
template <int PASS>
__global__ __launch_bounds__(256) void pool_edge_rows_kernel(
    const int* __restrict__ cnew, const int* __restrict__ segptr, const int* __restrict__ members,
    const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ w,
    const int* __restrict__ ncount, int nbound, int* __restrict__ cnt, const int* __restrict__ rowptr_c,
    int* __restrict__ row_c, int* __restrict__ col_c, float* __restrict__ w_c, int* __restrict__ overflow,
    int* __restrict__ total, int4* __restrict__ rowinfo, const int4* __restrict__ rowinfo_in) {
  const int lane = threadIdx.x & 63;
  const int A = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (PASS != 1 && blockIdx.x == 0 && threadIdx.x == 0) cnt[nbound] = 0;     // scan tail: rowptr_c[nbound] = total
  if (PASS == 1 && blockIdx.x == 0 && threadIdx.x == 0) *total = rowptr_c[nbound];
  if (A >= nbound) return;
  // requested before the coarse count is known (entries past it are never read back): one dependent load less
  int4 ri_in = make_int4(0, 0, 0, 0);
  if (PASS == 2 && rowinfo_in != nullptr) ri_in = rowinfo_in[A];
  const int nc = *ncount;
  if (A >= nc) { if (PASS != 1) cnt[A] = 0; return; }
  // the members' fine rows: PASS 0 walks segptr -> members -> rowptr (three dependent loads) and leaves the result
  // for PASS 1, whose chain then starts at the row entries
  int r0, d0, r1, d1;
  if (PASS == 2 && rowinfo_in != nullptr) {
    const int4 ri = ri_in;
    r0 = ri.x; d0 = ri.y; r1 = ri.z; d1 = ri.w;
    if (lane == 0) {
      rowinfo[A] = ri;
      if (d0 + d1 > 64) atomicOr(overflow, 1);
    }
  } else if (PASS != 1) {
    const int ms = segptr[A], me = segptr[A + 1];
    const int m0 = members[ms];
    const int m1 = (me - ms > 1) ? members[ms + 1] : -1;
    r0 = rowptr[m0]; d0 = rowptr[m0 + 1] - r0;
    r1 = m1 >= 0 ? rowptr[m1] : 0; d1 = m1 >= 0 ? rowptr[m1 + 1] - r1 : 0;
    if (lane == 0) {
      rowinfo[A] = make_int4(r0, d0, r1, d1);
      if (d0 + d1 > 64 || me - ms > 2) atomicOr(overflow, 1);
    }
  } else {
    const int4 ri = rowinfo[A];
    r0 = ri.x; d0 = ri.y; r1 = ri.z; d1 = ri.w;
  }
  int key = 0x7fffffff;
  float val = 0.f;
  if (lane < d0 + d1) {
    const int e = lane < d0 ? r0 + lane : r1 + (lane - d0);
    int k = cnew[col[e]];
    if (k != A) { key = k; val = w ? w[e] : 0.f; }
  }
  // bitonic sort, ascending by key; rows of up to 32 entries (the usual case: two mesh rows) skip the 64-wide merge.
  // Partner exchange at distance 1, 2, 4, 8 by DPP lane permutes (quad_perm, row_shl/shr:4, row_ror:8) -- 14 of the 15
  // stages of the 32-wide sort; a wave is a chain of ~20 dependent exchanges, and an LDS-crossbar permute costs ~10x
  // a DPP move in latency.  Every lane of the wave is active here (waves past the coarse count left as a whole).
  auto xchg = [&](int v, int j) -> int {
    switch (j) {
      case 1: return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);          // quad_perm [1,0,3,2]
      case 2: return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);          // quad_perm [2,3,0,1]
      case 4: {
        const int up = __builtin_amdgcn_update_dpp(0, v, 0x104, 0xf, 0xf, true);       // row_shl:4  lane i <- i + 4
        const int dn = __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);       // row_shr:4  lane i <- i - 4
        return (lane & 4) ? dn : up;
      }
      case 8: return __builtin_amdgcn_update_dpp(0, v, 0x128, 0xf, 0xf, true);          // row_ror:8 = xor 8 in a row
      default: return __shfl_xor(v, j, 64);
    }
  };
  auto stage = [&](int k, int j) {
    const int pk = xchg(key, j);
    const float pv = __int_as_float(xchg(__float_as_int(val), j));
    const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
    const bool take = keep_min ? (pk < key) : (pk > key);
    if (take) { key = pk; val = pv; }
  };
#pragma unroll
  for (int k = 2; k <= 32; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) stage(k, j);
  }
  if (d0 + d1 > 32) {                            // wave-uniform
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) stage(64, j);
  }
  const int prev = __shfl_up(key, 1, 64);
  const bool head = key != 0x7fffffff && (lane == 0 || prev != key);
  const unsigned long long hm = __ballot(head);
  if (PASS == 0) {
    if (lane == 0) cnt[A] = __popcll(hm);
    return;
  }
  if (PASS == 2 && lane == 0) cnt[A] = __popcll(hm);
  // run of duplicates starting at a head lane: up to the next head (or the first invalid lane)
  const unsigned long long vm = __ballot(key != 0x7fffffff);
  const int nvalid = __popcll(vm);
  const unsigned long long after = (lane >= 63) ? 0ull : (hm >> (lane + 1));
  const int next = after ? lane + 1 + (__ffsll((long long)after) - 1) : nvalid;
  const int len = head ? next - lane : 0;
  int maxlen = len;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, m, 64));
  double sum = (double)val;
  for (int t = 1; t < maxlen; ++t) {
    float v = __shfl_down(val, t, 64);
    if (t < len) sum += (double)v;
  }
  if (head) {
    const int t = __popcll(hm & ((1ull << lane) - 1ull));
    if (PASS == 2) {
      // one-pass form: the t-th unique entry parks in the t-th slot of the members' own fine rows (there are at most
      // d0 + d1 of them); pool_edge_compact_kernel moves the rows to their final places once the offsets are known
      const int pos = t < d0 ? r0 + t : r1 + (t - d0);
      col_c[pos] = key;                          // (col_c / w_c are the scratch pair here)
      if (w) w_c[pos] = (float)(sum / (double)len);
    } else {
      const int pos = rowptr_c[A] + t;
      row_c[pos] = A;
      col_c[pos] = key;
      if (w) w_c[pos] = (float)(sum / (double)len);
    }
  }
}

// second half of the one-pass form: 16 lanes per coarse node copy its parked entries to rowptr_c[A] ...
__global__ __launch_bounds__(256) void pool_edge_compact_kernel(const int* __restrict__ ncount, int nbound,
                                                                const int* __restrict__ rowptr_c,
                                                                const int4* __restrict__ rowinfo,
                                                                const int* __restrict__ tcol, const float* __restrict__ tw,
                                                                int* __restrict__ row_c, int* __restrict__ col_c,
                                                                float* __restrict__ w_c, int* __restrict__ total,
                                                                const int* publish_src, int* publish_host, int publish_seq) {
  const int A = (blockIdx.x * 256 + threadIdx.x) >> 4, k = threadIdx.x & 15;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int tot = rowptr_c[nbound];
    *total = tot;
    if (publish_host != nullptr) {
      // The sizes the host is waiting for are all final once this kernel has started (its own total included):
      // thread 0 hands them over through mapped host memory right away -- the host learns them while the copy pass
      // below is still running, without a device-to-host copy launch and a stream drain in between.
      for (int i = 0; i < 8; ++i) {
        const int* src = publish_src + i;
        publish_host[i] = (src == total) ? tot : *src;
      }
      __threadfence_system();
      __hip_atomic_store(publish_host + 8, publish_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  if (A >= nbound || A >= *ncount) return;
  const int o = rowptr_c[A], c = rowptr_c[A + 1] - o;
  const int4 ri = rowinfo[A];
  for (int t = k; t < c; t += 16) {
    const int src = t < ri.y ? ri.x + t : ri.z + (t - ri.y);
    row_c[o + t] = A;
    col_c[o + t] = tcol[src];
    if (tw) w_c[o + t] = tw[src];
  }
}

__global__ void pool_edge_rowptr_kernel(const uint64_t* __restrict__ ukeys, const int* __restrict__ count, int nmax,
                                        int bits, int* __restrict__ rowptr) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n > nmax) return;
  uint64_t target = (uint64_t)n << bits;
  int lo = 0, hi = *count;
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (ukeys[mid] < target) lo = mid + 1; else hi = mid;
  }
  rowptr[n] = lo;
}

struct EdgeRowsBuffers { CountScan cnt; int4* rowinfo; int* tcol; float* tw; };
// with E_fine (the fine edge count) the workspace also holds the scratch pair tcol, tw of the one-pass form
EdgeRowsBuffers carve_edge_rows(Arena& a, int64_t nbound, int64_t E_fine) {
  return {carve_count_scan(a, nbound + 1), a.take<int4>(nbound), E_fine > 0 ? a.take<int>(E_fine) : nullptr,
          E_fine > 0 ? a.take<float>(E_fine) : nullptr};
}
}  // namespace

size_t pool_edge_rows_ws_bytes_onepass(int64_t nbound, int64_t E) {
  return carve_bytes([&](Arena& a) { carve_edge_rows(a, nbound, E); });
}

// cnew, (segptr, members) = pair lists built with the bound `nbound` (fine node count), ncount = device
// count of coarse nodes.  rowptr_c has nbound + 1 entries; count[0] = coarse edges; overflow[0] |= 1 if
// some row did not fit (outputs are then incomplete and the caller must use pool_edge).
int pool_edge_rows(const int32_t* cnew, const int32_t* segptr, const int32_t* members, const int32_t* rowptr,
                   const int32_t* col, const float* w, const int32_t* ncount, int64_t nbound, int32_t* rowptr_c,
                   int32_t* row_c, int32_t* col_c, float* w_c, int32_t* count, int32_t* overflow, void* ws,
                   size_t ws_bytes, hipStream_t s, int64_t E_fine, const void* rowinfo_in, const int32_t* publish_src,
                   int32_t* publish_host, int publish_seq) {
  GEOBI_REQUIRE(nbound > 0, "pool_edge_rows: empty");
  Arena a(ws, ws_bytes);
  const EdgeRowsBuffers b = carve_edge_rows(a, nbound, E_fine);
  GEOBI_WS_CHECK("pool_edge_rows", a, ws, ws_bytes);
  int* cnt = b.cnt.cnt;
  int4* rowinfo = b.rowinfo;
  int blocks = cdiv(nbound, 4);
  if (E_fine > 0) {
    // one-pass form (callers that sized the workspace with pool_edge_rows_ws_bytes_onepass): gather + relabel + sort +
    // merge ONCE, entries parked in scratch, then a short copy pass instead of a second merge
    int* tcol = b.tcol;
    float* tw = b.tw;
    pool_edge_rows_kernel<2><<<blocks, 256, 0, s>>>(cnew, segptr, members, rowptr, col, w, ncount, (int)nbound, cnt,
                                                     nullptr, nullptr, tcol, tw, overflow, nullptr, rowinfo,
                                                     (const int4*)rowinfo_in);
    GEOBI_LAUNCH_OK();
    GEOBI_TRY(b.cnt.scan.run(cnt, rowptr_c, s));
    pool_edge_compact_kernel<<<cdiv(nbound * 16, 256), 256, 0, s>>>(ncount, (int)nbound, rowptr_c, rowinfo, tcol,
                                                                    w ? tw : nullptr, row_c, col_c, w_c, count,
                                                                    publish_src, publish_host, publish_seq);
    GEOBI_LAUNCH_OK();
    return 0;
  }
  pool_edge_rows_kernel<0><<<blocks, 256, 0, s>>>(cnew, segptr, members, rowptr, col, w, ncount, (int)nbound, cnt,
                                                   nullptr, nullptr, nullptr, nullptr, overflow, nullptr, rowinfo, nullptr);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.cnt.scan.run(cnt, rowptr_c, s));
  pool_edge_rows_kernel<1><<<blocks, 256, 0, s>>>(cnew, segptr, members, rowptr, col, w, ncount, (int)nbound, cnt,
                                                   rowptr_c, row_c, col_c, w_c, overflow, count, rowinfo, nullptr);
  GEOBI_LAUNCH_OK();
  return 0;
}

namespace {
struct PoolEdgeBuffers { uint64_t *k_in, *k_out, *ukeys; int *v_in, *v_out, *rank; CountScan head; PairSort<uint64_t, int> sort; };
PoolEdgeBuffers carve_pool_edge(Arena& a, int64_t E) {
  return {a.take<uint64_t>(E), a.take<uint64_t>(E), a.take<uint64_t>(E), a.take<int>(E), a.take<int>(E), a.take<int>(E),
          carve_count_scan(a, E), PairSort<uint64_t, int>::take(a, E)};
}
}  // namespace

size_t pool_edge_ws_bytes(int64_t E) { return carve_bytes([&](Arena& a) { carve_pool_edge(a, E); }); }

// Outputs are sized for the worst case (E entries, nmax + 1 row pointers); the true edge count is
// written to count[0] on the device.
int pool_edge(const int32_t* cnew, const int32_t* row, const int32_t* col, const float* w, int64_t E, int64_t nmax,
              int32_t* rowptr_c, int32_t* row_c, int32_t* col_c, float* w_c, int32_t* count, void* ws,
              size_t ws_bytes, hipStream_t s) {
  if (E <= 0) {
    GEOBI_HIP(hipMemsetAsync(rowptr_c, 0, sizeof(int) * (nmax + 1), s));
    GEOBI_HIP(hipMemsetAsync(count, 0, sizeof(int), s));
    return 0;
  }
  Arena a(ws, ws_bytes);
  const PoolEdgeBuffers b = carve_pool_edge(a, E);
  GEOBI_WS_CHECK("pool_edge", a, ws, ws_bytes);
  uint64_t *k_in = b.k_in, *k_out = b.k_out, *ukeys = b.ukeys;
  int *v_in = b.v_in, *v_out = b.v_out, *head = b.head.cnt, *rank = b.rank;
  int blocks = cdiv(E, 256);
  const int bits = key_bits(nmax);
  pool_edge_keys_kernel<<<blocks, 256, 0, s>>>(cnew, row, col, E, bits, k_in, v_in);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.sort.run(k_in, k_out, v_in, v_out, E, (unsigned)(2 * bits), s));
  pool_edge_heads_kernel<<<blocks, 256, 0, s>>>(k_out, E, head);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.head.scan.run(head, rank, s));
  pool_edge_emit_kernel<<<blocks, 256, 0, s>>>(k_out, v_out, head, rank, w, E, row_c, col_c, w_c, ukeys, count,
                                               bits);
  GEOBI_LAUNCH_OK();
  pool_edge_rowptr_kernel<<<cdiv(nmax + 1, 256), 256, 0, s>>>(ukeys, count, (int)nmax, bits, rowptr_c);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // namespace geobi

using namespace geobi;

extern "C" {

size_t geobi_pool_edge_rows_ws_bytes(int64_t nbound) { return pool_edge_rows_ws_bytes_onepass(nbound, 0); }
int geobi_pool_edge_rows(const int32_t* cnew, const int32_t* segptr, const int32_t* members, const int32_t* rowptr,
                         const int32_t* col, const float* w, const int32_t* ncount, int64_t nbound,
                         int32_t* rowptr_c, int32_t* row_c, int32_t* col_c, float* w_c, int32_t* count,
                         int32_t* overflow, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(nbound, 0);
  GEOBI_NOTNULL(cnew); GEOBI_NOTNULL(segptr); GEOBI_NOTNULL(members); GEOBI_NOTNULL(rowptr); GEOBI_NOTNULL(ncount);
  GEOBI_NOTNULL(rowptr_c); GEOBI_NOTNULL(row_c); GEOBI_NOTNULL(col_c); GEOBI_NOTNULL(count); GEOBI_NOTNULL(overflow);
  return pool_edge_rows(cnew, segptr, members, rowptr, col, w, ncount, nbound, rowptr_c, row_c, col_c, w_c, count,
                        overflow, ws, ws_bytes, as_stream(stream));
}

size_t geobi_debug_pool_edge_rows_onepass_ws_bytes(int64_t nbound, int64_t E) {
  return pool_edge_rows_ws_bytes_onepass(nbound, E);
}
int geobi_debug_pool_edge_rows_onepass(const int32_t* cnew, const int32_t* segptr, const int32_t* members,
                                       const int32_t* rowptr, const int32_t* col, const float* w, const int32_t* ncount,
                                       int64_t nbound, int64_t E_fine, const int32_t* rowinfo_in, int32_t* rowptr_c,
                                       int32_t* row_c, int32_t* col_c, float* w_c, int32_t* count, int32_t* overflow,
                                       void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(nbound, E_fine);
  GEOBI_REQUIRE(E_fine > 0, "%s: the one-pass form needs the fine edge count (E_fine = %lld)", __func__, (long long)E_fine);
  GEOBI_NOTNULL(cnew); GEOBI_NOTNULL(segptr); GEOBI_NOTNULL(members); GEOBI_NOTNULL(rowptr); GEOBI_NOTNULL(col);
  GEOBI_NOTNULL(ncount); GEOBI_NOTNULL(rowptr_c); GEOBI_NOTNULL(row_c); GEOBI_NOTNULL(col_c); GEOBI_NOTNULL(count);
  GEOBI_NOTNULL(overflow); GEOBI_NOTNULL(ws);
  if (w != nullptr) GEOBI_NOTNULL(w_c);
  return pool_edge_rows(cnew, segptr, members, rowptr, col, w, ncount, nbound, rowptr_c, row_c, col_c, w_c, count,
                        overflow, ws, ws_bytes, as_stream(stream), E_fine, rowinfo_in);
}

size_t geobi_pool_edge_ws_bytes(int64_t E) { return pool_edge_ws_bytes(E); }
int geobi_pool_edge(const int32_t* cnew, const int32_t* row, const int32_t* col, const float* w, int64_t E,
                    int64_t nmax, int32_t* rowptr_c, int32_t* row_c, int32_t* col_c, float* w_c, int32_t* count,
                    void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(nmax, E);
  GEOBI_NOTNULL(cnew); GEOBI_NOTNULL(rowptr_c); GEOBI_NOTNULL(count);
  return pool_edge(cnew, row, col, w, E, nmax, rowptr_c, row_c, col_c, w_c, count, ws, ws_bytes, as_stream(stream));
}

}  // extern "C"
