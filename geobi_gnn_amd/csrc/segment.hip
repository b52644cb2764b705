// What happens per cluster once match.hip has decided which nodes merge: the inverse lists cluster -> members and the
// reductions over them, with their entry points (PoolingLayer of the hot path, the reference's net_util.py:56-245).
//
//   segment_csr          inverse lists of any clustering  (sorted, deterministic)
//   segment_csr_pairs    the same for a matching, without a sort; segment_csr_compose chains two of them
//   segment_max/mean     feature pooling with arg-max for the backward        (scatter, net_util.py:131-134)
//   segment_sum          unpool backward; gather_rows is the unpool forward   (`x[unpooling_indices]`, :242-245)
//   segment_*2           the same reductions over the composition of a pooling layer's two matching steps
//
// The count-to-offset scans are CountScan records (device_steps.h); only segment_csr sorts (KeySort).
#include "../../include/geobi_hip.h"

#include "common.h"
#include "device_steps.h"

namespace geobi {

namespace {

// ------------------------------------------------------------------------ inverse lists
__global__ void seg_keys_kernel(const int* __restrict__ seg, int64_t n, int bits, uint64_t* __restrict__ keys) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keys[i] = ((uint64_t)(uint32_t)seg[i] << bits) | (uint64_t)(uint32_t)i;
}

__global__ void seg_unpack_kernel(const uint64_t* __restrict__ keys, int64_t n, int bits,
                                  int* __restrict__ members) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) members[i] = (int)(uint32_t)(keys[i] & ((1ull << bits) - 1));
}

__global__ void seg_ptr_kernel(const uint64_t* __restrict__ keys, int64_t n, int nseg, int bits,
                               int* __restrict__ segptr) {
  int sidx = blockIdx.x * blockDim.x + threadIdx.x;
  if (sidx > nseg) return;
  uint64_t target = (uint64_t)sidx << bits;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < target) lo = mid + 1; else hi = mid;
  }
  segptr[sidx] = (int)lo;
}

// Inverse lists of a MATCHING (clusters of <= 2 nodes, raw id = smaller member, cnew = dense id):
// no sort needed -- the representative takes slot 0, its partner slot 1 (members stay ascending).
__global__ void pair_count_kernel(const int* __restrict__ cnew, const int* __restrict__ raw, int N, int nseg,
                                  int* __restrict__ cnt) {
  int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < nseg) cnt[u] = 1;              // pass 1 of 2 (see launcher): every cluster has its representative
  (void)cnew; (void)raw; (void)N;
}

__global__ void pair_mark_kernel(const int* __restrict__ cnew, const int* __restrict__ raw, int N,
                                 int* __restrict__ cnt) {
  int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < N && raw[u] != u) cnt[cnew[u]] = 2;       // exactly one writer per matched cluster
}

__global__ void pair_fill_kernel(const int* __restrict__ cnew, const int* __restrict__ raw, int N, int nseg,
                                 int* __restrict__ segptr, int* __restrict__ members) {
  int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u == 0) segptr[nseg] = N;
  if (u < N) members[segptr[cnew[u]] + (raw[u] == u ? 0 : 1)] = u;
}

// Inverse lists of a composition  fine --(idx1)--> mid --(idx2)--> coarse :
// members12(C) = concat over m in members2(C) of members1(m)   (fixed order -> deterministic sums)
__global__ void compose_count_kernel(const int* __restrict__ segptr1, const int* __restrict__ segptr2,
                                     const int* __restrict__ members2, int nseg2, int* __restrict__ cnt) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nseg2) return;
  int n = 0;
  for (int e = segptr2[c]; e < segptr2[c + 1]; ++e) { int m = members2[e]; n += segptr1[m + 1] - segptr1[m]; }
  cnt[c] = n;
}

__global__ void compose_fill_kernel(const int* __restrict__ segptr1, const int* __restrict__ members1,
                                    const int* __restrict__ segptr2, const int* __restrict__ members2, int nseg2,
                                    int n_fine, int* __restrict__ segptr12, int* __restrict__ members12) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0) segptr12[nseg2] = n_fine;
  if (c >= nseg2) return;
  int o = segptr12[c];
  for (int e = segptr2[c]; e < segptr2[c + 1]; ++e) {
    int m = members2[e];
    for (int f = segptr1[m]; f < segptr1[m + 1]; ++f) members12[o++] = members1[f];
  }
}

// ----------------------------------------------------------------------- segment reduce
__global__ void segment_max_fwd_kernel(const float* __restrict__ x, int C, const int* __restrict__ segptr,
                                       const int* __restrict__ members, int nseg, float* __restrict__ out,
                                       int* __restrict__ arg) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nseg * C) return;
  int sidx = (int)(t / C), c = (int)(t % C);
  int rs = segptr[sidx], re = segptr[sidx + 1];
  float best = 0.f;          // empty segment -> 0 (torch_scatter fills untouched rows with 0)
  int bi = -1;
  for (int e = rs; e < re; ++e) {
    int m = members[e];      // members ascend, strict '>' keeps the first maximum
    float v = x[(size_t)m * C + c];
    if (bi < 0 || v > best) { best = v; bi = m; }
  }
  out[t] = best;
  arg[t] = bi;
}

// Max over the composition of two clusterings (a pooling layer's two matching steps) in ONE pass: segment c of the
// second step = concatenation, in order, of the first-step segments of its members.  The running maximum keeps the
// first maximum in that order -- the element the two-step form (max of the step-one maxima, first maximum at each
// step) routes to -- so out and the backward's routing are identical to two segment_max passes; the step-one
// maxima are never materialised.  arg12 holds the FINE row of the maximum.
__global__ void segment_max2_fwd_kernel(const float* __restrict__ x, int C, const int* __restrict__ segptr1,
                                        const int* __restrict__ members1, const int* __restrict__ segptr2,
                                        const int* __restrict__ members2, int nseg2, float* __restrict__ out,
                                        int* __restrict__ arg12) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nseg2 * C) return;
  const int sidx = (int)(t / C), c = (int)(t % C);
  float best = 0.f;
  int bi = -1;
  for (int e2 = segptr2[sidx]; e2 < segptr2[sidx + 1]; ++e2) {
    const int m = members2[e2];
    float mb = 0.f;                               // the step-one maximum of segment m and its first position
    int mi = -1;
    for (int e1 = segptr1[m]; e1 < segptr1[m + 1]; ++e1) {
      const int f = members1[e1];
      const float v = x[(size_t)f * C + c];
      if (mi < 0 || v > mb) { mb = v; mi = f; }
    }
    if (mi >= 0 && (bi < 0 || mb > best)) { best = mb; bi = mi; }
  }
  out[t] = best;
  arg12[t] = bi;
}

// gather form of its backward: fine row n receives the gradient of its composed segment where it was the arg-max
__global__ void segment_max2_bwd_kernel(const float* __restrict__ gout, const int* __restrict__ arg12,
                                        const int* __restrict__ seg12, int C, int64_t total, int nseg2,
                                        float* __restrict__ gx, int add) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int n = (int)(t / C), c = (int)(t % C);
  const int sg = seg12[n];
  float v = 0.f;
  if (sg >= 0 && sg < nseg2) {
    const size_t o = (size_t)sg * C + c;
    if (arg12[o] == n) v = gout[o];
  }
  gx[t] = add ? gx[t] + v : v;                  // add: on top of what gx holds (a skip connection's gradient)
}

// gather form: fine row n receives the gradient of its segment where it was the arg-max (every
// element of gx is written exactly once -> no zero-fill pass)
__global__ void segment_max_bwd_kernel(const float* __restrict__ gout, const int* __restrict__ arg,
                                       const int* __restrict__ seg, int C, int64_t total, int nseg,
                                       float* __restrict__ gx) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  int n = (int)(t / C), c = (int)(t % C);
  int sg = seg[n];
  float v = 0.f;
  if (sg >= 0 && sg < nseg) {
    size_t o = (size_t)sg * C + c;
    if (arg[o] == n) v = gout[o];
  }
  gx[t] = v;
}

__global__ void segment_sum_kernel(const float* __restrict__ x, int C, const int* __restrict__ segptr,
                                   const int* __restrict__ members, int nseg, int mean, float* __restrict__ out) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nseg * C) return;
  int sidx = (int)(t / C), c = (int)(t % C);
  int rs = segptr[sidx], re = segptr[sidx + 1];
  float s = 0.f;
  for (int e = rs; e < re; ++e) s += x[(size_t)members[e] * C + c];
  if (mean) s = s / (float)max(re - rs, 1);
  out[t] = s;
}

// Sum over the composition of two clusterings, the members walked in the order the composed list (compose_fill_kernel)
// would hold them -- same sums bit for bit, without building that list.
__global__ void segment_sum2_kernel(const float* __restrict__ x, int C, const int* __restrict__ segptr1,
                                    const int* __restrict__ members1, const int* __restrict__ segptr2,
                                    const int* __restrict__ members2, int nseg2, float* __restrict__ out) {
  // four channels per thread (16-B loads; C is 64 or 128 on the path), same summation order per channel as before
  const int Q = C >> 2;
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nseg2 * Q) return;
  const int sidx = (int)(t / Q), c = (int)(t % Q) * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int e2 = segptr2[sidx]; e2 < segptr2[sidx + 1]; ++e2) {
    const int m = members2[e2];
    for (int e1 = segptr1[m]; e1 < segptr1[m + 1]; ++e1) {
      const float4 v = *reinterpret_cast<const float4*>(x + (size_t)members1[e1] * C + c);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  *reinterpret_cast<float4*>(out + (size_t)sidx * C + c) = s;
}

__global__ void segment_mean_bwd_kernel(const float* __restrict__ gout, const int* __restrict__ seg,
                                        const int* __restrict__ segptr, int C, int64_t total,
                                        float* __restrict__ gx) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  int n = (int)(t / C), c = (int)(t % C);
  int sidx = seg[n];
  gx[t] = gout[(size_t)sidx * C + c] / (float)max(segptr[sidx + 1] - segptr[sidx], 1);
}

__global__ void gather_rows_kernel(const float* __restrict__ x, const int* __restrict__ idx, int C, int64_t total,
                                   float* __restrict__ out) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  int n = (int)(t / C), c = (int)(t % C);
  out[t] = x[(size_t)idx[n] * C + c];
}

struct KeySortBuffers { uint64_t *k_in, *k_out; KeySort<uint64_t> sort; };
KeySortBuffers carve_key_sort(Arena& a, int64_t n) {
  return {a.take<uint64_t>(n), a.take<uint64_t>(n), KeySort<uint64_t>::take(a, n)};
}

}  // namespace

// ---- the launchers executor.hip calls too (prototypes in common.h)
int segment_max2_fwd(const float* x, int C, const int32_t* segptr1, const int32_t* members1, const int32_t* segptr2,
                     const int32_t* members2, int64_t nseg2, float* out, int32_t* arg12, hipStream_t s) {
  if (nseg2 <= 0) return 0;
  segment_max2_fwd_kernel<<<cdiv(nseg2 * C, 256), 256, 0, s>>>(x, C, segptr1, members1, segptr2, members2, (int)nseg2, out,
                                                              arg12);
  GEOBI_LAUNCH_OK();
  return 0;
}

int segment_max2_bwd(const float* gout, const int32_t* arg12, const int32_t* seg12, int C, int64_t nseg2, int64_t n_fine,
                     float* gx, int add, hipStream_t s) {
  if (n_fine <= 0) return 0;
  segment_max2_bwd_kernel<<<cdiv(n_fine * C, 256), 256, 0, s>>>(gout, arg12, seg12, C, n_fine * C, (int)nseg2, gx, add);
  GEOBI_LAUNCH_OK();
  return 0;
}

int segment_sum(const float* x, int C, const int32_t* segptr, const int32_t* members, int64_t nseg, int mean,
                float* out, hipStream_t s) {
  if (nseg <= 0) return 0;
  segment_sum_kernel<<<cdiv(nseg * C, 256), 256, 0, s>>>(x, C, segptr, members, (int)nseg, mean, out);
  GEOBI_LAUNCH_OK();
  return 0;
}

int segment_sum2(const float* x, int C, const int32_t* segptr1, const int32_t* members1, const int32_t* segptr2,
                 const int32_t* members2, int64_t nseg2, float* out, hipStream_t s) {
  if (nseg2 <= 0) return 0;
  GEOBI_REQUIRE((C & 3) == 0, "segment_sum2: channel count %d is not a multiple of 4", C);
  segment_sum2_kernel<<<cdiv(nseg2 * (C >> 2), 256), 256, 0, s>>>(x, C, segptr1, members1, segptr2, members2, (int)nseg2, out);
  GEOBI_LAUNCH_OK();
  return 0;
}

int segment_mean_bwd(const float* gout, const int32_t* seg, const int32_t* segptr, int C, int64_t n_fine, float* gx,
                     hipStream_t s) {
  if (n_fine <= 0) return 0;
  segment_mean_bwd_kernel<<<cdiv(n_fine * C, 256), 256, 0, s>>>(gout, seg, segptr, C, n_fine * C, gx);
  GEOBI_LAUNCH_OK();
  return 0;
}

int gather_rows(const float* x, const int32_t* idx, int C, int64_t n_out, float* out, hipStream_t s) {
  if (n_out <= 0) return 0;
  gather_rows_kernel<<<cdiv(n_out * C, 256), 256, 0, s>>>(x, idx, C, n_out * C, out);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // namespace geobi

using namespace geobi;

extern "C" {

size_t geobi_segment_csr_ws_bytes(int64_t n) { return carve_bytes([&](Arena& a) { carve_key_sort(a, n); }); }

int geobi_segment_csr(const int32_t* seg, int64_t n, int64_t nseg, int32_t* segptr, int32_t* members, void* ws,
                      size_t ws_bytes, void* stream) {
  GEOBI_SIZES(nseg, n);          // n counts list entries (3 F corners of a face table): an edge-like count
  GEOBI_NOTNULL(segptr);
  hipStream_t s = as_stream(stream);
  if (n <= 0) {
    GEOBI_HIP(hipMemsetAsync(segptr, 0, sizeof(int) * (nseg + 1), s));
    return 0;
  }
  Arena a(ws, ws_bytes);
  const KeySortBuffers b = carve_key_sort(a, n);
  GEOBI_WS_CHECK("segment_csr", a, ws, ws_bytes);
  uint64_t *k_in = b.k_in, *k_out = b.k_out;
  const int bits = key_bits(n);                 // member index < n
  const int sbits = key_bits(nseg);
  seg_keys_kernel<<<cdiv(n, 256), 256, 0, s>>>(seg, n, bits, k_in);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.sort.run(k_in, k_out, n, (unsigned)(bits + sbits), s));
  seg_unpack_kernel<<<cdiv(n, 256), 256, 0, s>>>(k_out, n, bits, members);
  seg_ptr_kernel<<<cdiv(nseg + 1, 256), 256, 0, s>>>(k_out, n, (int)nseg, bits, segptr);
  GEOBI_LAUNCH_OK();
  return 0;
}

size_t geobi_segment_pairs_ws_bytes(int64_t nseg) { return carve_bytes([&](Arena& a) { carve_count_scan(a, nseg); }); }

int geobi_segment_csr_pairs(const int32_t* cnew, const int32_t* raw, int64_t N, int64_t nseg, int32_t* segptr,
                            int32_t* members, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(N, 0);
  GEOBI_NOTNULL(cnew); GEOBI_NOTNULL(raw); GEOBI_NOTNULL(segptr); GEOBI_NOTNULL(members);
  hipStream_t s = as_stream(stream);
  GEOBI_REQUIRE(N > 0 && nseg > 0, "segment_csr_pairs: empty");
  Arena a(ws, ws_bytes);
  const CountScan c = carve_count_scan(a, nseg);
  GEOBI_WS_CHECK("segment_csr_pairs", a, ws, ws_bytes);
  int* cnt = c.cnt;
  pair_count_kernel<<<cdiv(nseg, 256), 256, 0, s>>>(cnew, raw, (int)N, (int)nseg, cnt);
  pair_mark_kernel<<<cdiv(N, 256), 256, 0, s>>>(cnew, raw, (int)N, cnt);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(c.scan.run(cnt, segptr, s));
  pair_fill_kernel<<<cdiv(N, 256), 256, 0, s>>>(cnew, raw, (int)N, (int)nseg, segptr, members);
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_segment_csr_compose(const int32_t* segptr1, const int32_t* members1, const int32_t* segptr2,
                              const int32_t* members2, int64_t nseg2, int64_t n_fine, int32_t* segptr12,
                              int32_t* members12, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(n_fine, 0);
  GEOBI_NOTNULL(segptr1); GEOBI_NOTNULL(members1); GEOBI_NOTNULL(segptr2); GEOBI_NOTNULL(members2);
  GEOBI_NOTNULL(segptr12); GEOBI_NOTNULL(members12);
  hipStream_t s = as_stream(stream);
  GEOBI_REQUIRE(nseg2 > 0, "segment_csr_compose: empty");
  Arena a(ws, ws_bytes);
  const CountScan c = carve_count_scan(a, nseg2);
  GEOBI_WS_CHECK("segment_csr_compose", a, ws, ws_bytes);
  int* cnt = c.cnt;
  compose_count_kernel<<<cdiv(nseg2, 256), 256, 0, s>>>(segptr1, segptr2, members2, (int)nseg2, cnt);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(c.scan.run(cnt, segptr12, s));
  compose_fill_kernel<<<cdiv(nseg2, 256), 256, 0, s>>>(segptr1, members1, segptr2, members2, (int)nseg2,
                                                       (int)n_fine, segptr12, members12);
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_segment_max_fwd(const float* x, int C, const int32_t* segptr, const int32_t* members, int64_t nseg,
                          float* out, int32_t* arg, void* stream) {
  GEOBI_SIZES(nseg, 0);
  hipStream_t s = as_stream(stream);
  if (nseg <= 0) return 0;
  segment_max_fwd_kernel<<<cdiv(nseg * C, 256), 256, 0, s>>>(x, C, segptr, members, (int)nseg, out, arg);
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_segment_max_bwd(const float* gout, const int32_t* arg, const int32_t* seg, int C, int64_t nseg,
                          int64_t n_fine, float* gx, void* stream) {
  GEOBI_SIZES(n_fine, 0);
  hipStream_t s = as_stream(stream);
  if (n_fine <= 0) return 0;
  segment_max_bwd_kernel<<<cdiv(n_fine * C, 256), 256, 0, s>>>(gout, arg, seg, C, n_fine * C, (int)nseg, gx);
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_debug_segment_max2_fwd(const float* x, int C, const int32_t* segptr1, const int32_t* members1,
                                 const int32_t* segptr2, const int32_t* members2, int64_t nseg2, float* out,
                                 int32_t* arg12, void* stream) {
  GEOBI_SIZES(nseg2, 0);
  GEOBI_REQUIRE(C > 0, "%s: C = %d", __func__, C);
  if (nseg2 > 0) {
    GEOBI_NOTNULL(x); GEOBI_NOTNULL(segptr1); GEOBI_NOTNULL(members1); GEOBI_NOTNULL(segptr2); GEOBI_NOTNULL(members2);
    GEOBI_NOTNULL(out); GEOBI_NOTNULL(arg12);
  }
  return segment_max2_fwd(x, C, segptr1, members1, segptr2, members2, nseg2, out, arg12, as_stream(stream));
}

int geobi_debug_segment_max2_bwd(const float* gout, const int32_t* arg12, const int32_t* seg12, int C, int64_t nseg2,
                                 int64_t n_fine, float* gx, int add, void* stream) {
  GEOBI_SIZES(n_fine, 0);
  GEOBI_SIZES(nseg2, 0);
  GEOBI_REQUIRE(C > 0, "%s: C = %d", __func__, C);
  if (n_fine > 0) { GEOBI_NOTNULL(gout); GEOBI_NOTNULL(arg12); GEOBI_NOTNULL(seg12); GEOBI_NOTNULL(gx); }
  return segment_max2_bwd(gout, arg12, seg12, C, nseg2, n_fine, gx, add, as_stream(stream));
}

int geobi_debug_segment_sum2(const float* x, int C, const int32_t* segptr1, const int32_t* members1,
                             const int32_t* segptr2, const int32_t* members2, int64_t nseg2, float* out, void* stream) {
  GEOBI_SIZES(nseg2, 0);
  GEOBI_REQUIRE(C > 0, "%s: C = %d", __func__, C);
  if (nseg2 > 0) {
    GEOBI_NOTNULL(x); GEOBI_NOTNULL(segptr1); GEOBI_NOTNULL(members1); GEOBI_NOTNULL(segptr2); GEOBI_NOTNULL(members2);
    GEOBI_NOTNULL(out);
  }
  return segment_sum2(x, C, segptr1, members1, segptr2, members2, nseg2, out, as_stream(stream));
}

int geobi_segment_sum(const float* x, int C, const int32_t* segptr, const int32_t* members, int64_t nseg, int mean,
                      float* out, void* stream) {
  GEOBI_SIZES(nseg, 0);
  return segment_sum(x, C, segptr, members, nseg, mean, out, as_stream(stream));
}

int geobi_segment_mean_bwd(const float* gout, const int32_t* seg, const int32_t* segptr, int C, int64_t n_fine,
                           float* gx, void* stream) {
  GEOBI_SIZES(n_fine, 0);
  return segment_mean_bwd(gout, seg, segptr, C, n_fine, gx, as_stream(stream));
}

int geobi_gather_rows(const float* x, const int32_t* idx, int C, int64_t n_out, float* out, void* stream) {
  GEOBI_SIZES(n_out, 0);
  return gather_rows(x, idx, C, n_out, out, as_stream(stream));
}

}  // extern "C"
