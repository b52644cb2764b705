// Edge-sorted adjacency (CSR) construction for the mesh graphs.
//
// The reference hands the path COO `edge_index [2,E] int64` (row = source j, col = target i;
// /root/reference/code/network.py:271 -> FeaStConv).  Every kernel of this library walks a
// CSR sorted by (segment node, neighbour) so gathers are row-coalesced and aggregation is a
// sorted-segment reduction (no atomics, fixed summation order -> bitwise reproducible).
// Self loops are dropped here: FeaStConv removes and re-adds exactly one per node, which
// the conv kernels apply implicitly, and the pooling layer drops them first too
// (/root/reference/code/net_util.py:163).
//
// Also here, with their entry points: the batched union copy (geobi_concat32) and the two index builders of the pooled
// graphs, geobi_expand_rowptr (CSR row pointers -> one row id per edge) and geobi_gather_f32.
#include "common.h"
#include "device_steps.h"
#include "../../include/geobi_hip.h"

#include <cstring>

namespace geobi {

namespace {

__global__ void make_keys_kernel(const int64_t* __restrict__ seg, const int64_t* __restrict__ nbr, int64_t E,
                                 int64_t N, int drop_self, int bits, uint64_t* __restrict__ keys,
                                 int32_t* __restrict__ vals, int32_t* __restrict__ bad) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  int64_t a = seg[e], b = nbr[e];
  const bool ok = a >= 0 && a < N && b >= 0 && b < N;       // ids outside [0, N) never reach the kernels
  if (!ok && bad != nullptr) atomicAdd(bad, 1);
  keys[e] = (!ok || (drop_self && a == b)) ? kSentinel : (((uint64_t)a << bits) | (uint64_t)(uint32_t)b);
  vals[e] = (int32_t)e;
}

__global__ void expand_keys_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int N,
                                   int64_t Ecap, int bits, uint64_t* __restrict__ keys, int32_t* __restrict__ vals) {
  // one thread per node: emits (col << 32 | row) for its CSR segment
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < N) {
    int rs = rowptr[n], re = rowptr[n + 1];
    for (int e = rs; e < re; ++e) {
      keys[e] = ((uint64_t)(uint32_t)col[e] << bits) | (uint64_t)(uint32_t)n;
      vals[e] = e;
    }
  }
  // tail [rowptr[N], Ecap) is padding
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)gridDim.x * blockDim.x;
  int64_t E = rowptr[N];
  for (int64_t e = E + t; e < Ecap; e += total) {
    keys[e] = kSentinel;
    vals[e] = -1;
  }
}

__global__ void unpack_sorted_kernel(const uint64_t* __restrict__ keys, int64_t E, int bits,
                                     int32_t* __restrict__ col) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  uint64_t k = keys[e];
  col[e] = (k == kSentinel) ? -1 : (int32_t)(uint32_t)(k & ((1ull << bits) - 1));
}

// rowptr[n] = first position whose key >= (n << 32)   (n = N gives the valid edge count)
__global__ void rowptr_search_kernel(const uint64_t* __restrict__ keys, int64_t E, int N, int bits,
                                     int32_t* __restrict__ rowptr) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n > N) return;
  uint64_t target = (uint64_t)n << bits;
  int64_t lo = 0, hi = E;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < target) lo = mid + 1; else hi = mid;
  }
  rowptr[n] = (int32_t)lo;
}

__global__ void invert_perm_kernel(const int32_t* __restrict__ pos, int64_t Ecap, const int32_t* __restrict__ count,
                                   int32_t* __restrict__ inv) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= Ecap) return;
  if (e < *count) inv[pos[e]] = (int32_t)e;
}

// For every edge (i -> j) of a (row, col)-sorted CSR: the position of (j -> i), or -1 (and flag |= 1) if
// the reverse edge is missing.  For a symmetric graph the transposed CSR is the CSR itself and this
// index is the edge correspondence the backward pass needs -- no sort.
__global__ void reverse_index_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ row,
                                     const int32_t* __restrict__ col, int64_t E, int32_t* __restrict__ pos_rev,
                                     int32_t* __restrict__ flag) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  int i = row[e], j = col[e];
  int lo = rowptr[j], hi = rowptr[j + 1];
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    if (col[mid] < i) lo = mid + 1; else hi = mid;
  }
  if (lo < rowptr[j + 1] && col[lo] == i) {
    pos_rev[e] = lo;
  } else {
    pos_rev[e] = -1;
    if (flag) atomicOr(flag, 1);
  }
}

struct SortBuffers { uint64_t *k_in, *k_out; int32_t *v_in, *v_out; PairSort<uint64_t, int32_t> sort; };
SortBuffers carve_sort(Arena& a, int64_t E) {
  return {a.take<uint64_t>(E), a.take<uint64_t>(E), a.take<int32_t>(E), a.take<int32_t>(E),
          PairSort<uint64_t, int32_t>::take(a, E)};
}

// ---------------------------------------------------------------- batched union copy (geobi_concat32)
constexpr int kMaxSegs = 96;
struct ConcatJob {
  const uint32_t* src[kMaxSegs];
  uint32_t* dst[kMaxSegs];
  int64_t start[kMaxSegs + 1];     // element offsets of the jobs in the launch's index space
  uint32_t fill[kMaxSegs];         // int32 add, or the bits of the float fill value
  int n, is_float;
};

// One launch for every array of a union batch: 4 elements per thread and step; the job of an element is found by a
// binary search (find_part, common.h) over <= 96 start offsets held in LDS.
__global__ __launch_bounds__(256) void concat32_kernel(ConcatJob job) {
  __shared__ int64_t s_start[kMaxSegs + 1];
  for (int i = threadIdx.x; i <= job.n; i += 256) s_start[i] = job.start[i];
  __syncthreads();
  const int64_t total = s_start[job.n];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int lo = find_part(s_start, job.n, i);
    const int64_t k = i - s_start[lo];
    const uint32_t* src = job.src[lo];
    uint32_t v = job.fill[lo];
    if (src != nullptr) v = job.is_float ? src[k] : src[k] + v;
    job.dst[lo][k] = v;
  }
}

// ---------------------------------------------------------------- index builders of the pooled graphs
__global__ void expand_rowptr_kernel(const int* __restrict__ rowptr, int N, int* __restrict__ row) {
  int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  for (int e = rowptr[n]; e < rowptr[n + 1]; ++e) row[e] = n;
}

__global__ void gather_f32_kernel(const float* __restrict__ src, const int* __restrict__ idx, int64_t n,
                                  float* __restrict__ dst) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { int k = idx[i]; dst[i] = k >= 0 ? src[k] : 0.f; }
}

}  // namespace

// executor.hip calls it too: the one launcher of this unit with a prototype in common.h
int csr_reverse_index(const int32_t* rowptr, const int32_t* row, const int32_t* col, int64_t E, int32_t* pos_rev,
                      int32_t* flag, hipStream_t s) {
  if (flag != nullptr) GEOBI_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
  if (E <= 0) return 0;
  reverse_index_kernel<<<cdiv(E, 256), 256, 0, s>>>(rowptr, row, col, E, pos_rev, flag);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // namespace geobi

using namespace geobi;

extern "C" {

size_t geobi_csr_ws_bytes(int64_t E, int64_t N) {
  (void)N;
  return carve_bytes([&](Arena& a) { carve_sort(a, E); });
}

int geobi_csr_from_coo(const int64_t* seg, const int64_t* nbr, int64_t E, int64_t N, int drop_self, int32_t* rowptr,
                       int32_t* col, int32_t* eid, int32_t* bad, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(N, E);
  GEOBI_NOTNULL(rowptr);
  if (E > 0) { GEOBI_NOTNULL(seg); GEOBI_NOTNULL(nbr); GEOBI_NOTNULL(col); GEOBI_NOTNULL(eid); }
  hipStream_t s = as_stream(stream);
  GEOBI_REQUIRE(N >= 0 && E >= 0 && N < (1ll << 31) && E < (1ll << 31), "csr_from_coo: sizes out of int32 range");
  if (bad != nullptr) GEOBI_HIP(hipMemsetAsync(bad, 0, sizeof(int32_t), s));
  if (E == 0) {
    GEOBI_HIP(hipMemsetAsync(rowptr, 0, sizeof(int32_t) * (N + 1), s));
    return 0;
  }
  Arena a(ws, ws_bytes);
  const SortBuffers sb = carve_sort(a, E);
  GEOBI_WS_CHECK("csr_from_coo", a, ws, ws_bytes);
  const int T = 256;
  const int bits = key_bits(N);
  make_keys_kernel<<<cdiv(E, T), T, 0, s>>>(seg, nbr, E, N, drop_self, bits, sb.k_in, sb.v_in, bad);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(sb.sort.run(sb.k_in, sb.k_out, sb.v_in, eid, E, (unsigned)(2 * bits), s));
  unpack_sorted_kernel<<<cdiv(E, T), T, 0, s>>>(sb.k_out, E, bits, col);
  GEOBI_LAUNCH_OK();
  rowptr_search_kernel<<<cdiv(N + 1, T), T, 0, s>>>(sb.k_out, E, (int)N, bits, rowptr);
  GEOBI_LAUNCH_OK();
  return 0;
}

// Transposed CSR of a CSR whose valid edge count lives on the device (rowptr[N]); `Ecap` is the
// allocated length of col.  pos_t[e_t] = position of that edge in the input CSR; inv_pos[e] =
// position of input edge e in the transposed CSR.
int geobi_csr_transpose(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t Ecap, int32_t* rowptr_t,
                        int32_t* col_t, int32_t* pos_t, int32_t* inv_pos, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(N, Ecap);
  GEOBI_NOTNULL(rowptr); GEOBI_NOTNULL(rowptr_t);
  if (Ecap > 0) { GEOBI_NOTNULL(col); GEOBI_NOTNULL(col_t); GEOBI_NOTNULL(pos_t); }
  hipStream_t s = as_stream(stream);
  if (Ecap == 0) {
    GEOBI_HIP(hipMemsetAsync(rowptr_t, 0, sizeof(int32_t) * (N + 1), s));
    return 0;
  }
  Arena a(ws, ws_bytes);
  const SortBuffers sb = carve_sort(a, Ecap);
  GEOBI_WS_CHECK("csr_transpose", a, ws, ws_bytes);
  const int T = 256;
  int blocks = cdiv(N > 0 ? N : 1, T);
  const int bits = key_bits(N);
  expand_keys_kernel<<<blocks, T, 0, s>>>(rowptr, col, (int)N, Ecap, bits, sb.k_in, sb.v_in);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(sb.sort.run(sb.k_in, sb.k_out, sb.v_in, pos_t, Ecap, (unsigned)(2 * bits), s));
  // low 32 bits of the transposed key hold the original row = the neighbour in the transposed view
  unpack_sorted_kernel<<<cdiv(Ecap, T), T, 0, s>>>(sb.k_out, Ecap, bits, col_t);
  GEOBI_LAUNCH_OK();
  rowptr_search_kernel<<<cdiv(N + 1, T), T, 0, s>>>(sb.k_out, Ecap, (int)N, bits, rowptr_t);
  GEOBI_LAUNCH_OK();
  if (inv_pos) {
    invert_perm_kernel<<<cdiv(Ecap, T), T, 0, s>>>(pos_t, Ecap, rowptr + N, inv_pos);
    GEOBI_LAUNCH_OK();
  }
  return 0;
}

int geobi_csr_reverse_index(const int32_t* rowptr, const int32_t* row, const int32_t* col, int64_t E,
                            int32_t* pos_rev, int32_t* flag, void* stream) {
  GEOBI_SIZES(0, E);
  GEOBI_NOTNULL(rowptr);                         // flag may be NULL: the caller knows the graph is symmetric
  if (E > 0) { GEOBI_NOTNULL(row); GEOBI_NOTNULL(col); GEOBI_NOTNULL(pos_rev); }
  return csr_reverse_index(rowptr, row, col, E, pos_rev, flag, as_stream(stream));
}

int geobi_expand_rowptr(const int32_t* rowptr, int64_t N, int32_t* row, void* stream) {
  GEOBI_SIZES(N, 0);
  hipStream_t s = as_stream(stream);
  if (N <= 0) return 0;
  expand_rowptr_kernel<<<cdiv(N, 256), 256, 0, s>>>(rowptr, (int)N, row);
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_concat32(const geobi_copy_seg_t* segs, int n_segs, int is_float, void* stream) {
  if (n_segs <= 0) return 0;
  GEOBI_NOTNULL(segs);
  hipStream_t s = as_stream(stream);
  for (int base = 0; base < n_segs; base += kMaxSegs) {
    ConcatJob job;
    job.n = n_segs - base < kMaxSegs ? n_segs - base : kMaxSegs;
    job.is_float = is_float;
    job.start[0] = 0;
    for (int i = 0; i < job.n; ++i) {
      const geobi_copy_seg_t& g = segs[base + i];
      GEOBI_REQUIRE(g.n >= 0 && (g.n == 0 || g.dst != nullptr), "concat32: bad segment %d", base + i);
      job.src[i] = (const uint32_t*)g.src;
      job.dst[i] = (uint32_t*)g.dst;
      uint32_t bits;
      if (is_float) memcpy(&bits, &g.value, 4); else bits = (uint32_t)g.add;
      job.fill[i] = bits;
      job.start[i + 1] = job.start[i] + g.n;
    }
    const int64_t total = job.start[job.n];
    if (total == 0) continue;
    int64_t blocks = (total + 1023) / 1024;
    if (blocks > 4096) blocks = 4096;
    concat32_kernel<<<(int)blocks, 256, 0, s>>>(job);
    GEOBI_LAUNCH_OK();
  }
  return 0;
}

int geobi_gather_f32(const float* src, const int32_t* idx, int64_t n, float* dst, void* stream) {
  GEOBI_SIZES(0, n);
  hipStream_t s = as_stream(stream);
  if (n <= 0) return 0;
  gather_f32_kernel<<<cdiv(n, 256), 256, 0, s>>>(src, idx, n, dst);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
