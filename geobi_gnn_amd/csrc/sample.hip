// Points drawn uniformly by area on a mesh surface: integer face weights and their inclusive scan, then one
// Philox call, one upper-bound search and one barycentric combination per sample.
//
// The reference has no call site for this: every distance of its evaluation starts from a vertex
// (code/data_util.py:584-616).  A CAD face of a few large triangles has no vertex inside it; samples do.
//
// Weights (sample_weights), integer-exact so that two runs, two grid shapes and the host model agree on every face:
//   d[f]       |e1 x e2| of the float32 corners widened to fp64, every product and difference rounded on its own (no FMA
//              contraction, "as numpy does"); a non-finite d counts as 0
//   dmax       max_f d by a fixed-shape reduction (a block's LDS tree, then one block over the blocks' maxima)
//   e          frexp(dmax) = m * 2^e; exponent[0] = e (0 for dmax == 0)
//   weight[f]  floor(ldexp(d[f], 32 - e)): the largest face lands in [2^31, 2^32), a face below 2^-32 of it gets 0
//   cum        inclusive scan of weight in 64-bit integers (rocPRIM; integer sums are exact in any order), < 2^56
//
// Draw (sample_surface): sample i uses the counter (first + i, stream_id, draw, 2) -- blocks 0 and 1 are noise.hip's --
// and the key (seed lo, seed hi).  r = w0 << 32 | w1, t = umul64hi(r, total) with total = cum[F - 1] read on the device,
// face = the first f with cum[f] > t (an upper bound: zero-weight faces, runs of equal cum, are never chosen);
// u1 = uniform(w2), u2 = uniform(w3), folded into the triangle (u1 + u2 > 1: both become 1 - u); b = (1 - u1 - u2, u1, u2)
// is exact in fp32 for uniforms of the form (k + 0.5) 2^-23; p = fma(b2, c, fma(b1, b, b0 * a)).  total == 0: face -1, zeros.
//
// Shape of the search: a block stages kTable evenly spaced entries of cum in LDS (16 KB; all of cum for F <= kTable),
// finds the bucket there and finishes inside it from global memory: log2(F / kTable) dependent global loads per sample
// instead of log2 F.  The bucket bounds are entries of cum themselves, so the result is that of the plain search.  One
// thread per sample, grid-stride; plain vector stores, no atomics.  Corner ids are clamped into [0, V): a foreign table
// never reads outside points.
//
// Union batch (sample_weights_parts, sample_surface_parts): fv holds global vertex ids, fptr[P + 1] cuts its
// rows into parts.  Workgroups are formed per part, as dist.hip's nearest_parts_kernel forms them; the part table rides in
// the kernel arguments, kMaxParts parts per launch.  Every part gets its own dmax and exponent; cum is ONE inclusive scan
// over the union's weights into the workspace minus the part's base (the scan's entry before the part's first row):
// integer sums are exact, so the rows of part p hold what sample_weights gives on that mesh alone.  The draw of part p is
// draw_rows over the part's slice of cum with the part's stream id: the single-mesh rows, the face plus fptr[p].
#include "common.h"
#include "../../include/geobi_hip.h"
#include "philox.h"
#include "device_steps.h"

#include <math.h>

namespace geobi {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;                    // 256 CUs x 4 workgroups; the rest by grid stride
constexpr int kTable = 2048;                        // LDS table of the draw: 2048 x 8 bytes = 16 KB

__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// max over the block, every thread gets it: an LDS tree of fixed shape (a maximum does not depend on it anyway)
__device__ __forceinline__ double block_max_fp64(double v) {
  __shared__ double s[kThreads];
  s[threadIdx.x] = v;
  __syncthreads();
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) s[threadIdx.x] = fmax(s[threadIdx.x], s[threadIdx.x + h]);
    __syncthreads();
  }
  return s[0];
}

// d[f] = |e1 x e2| of face f: float32 corners widened to fp64, every product and difference rounded on its own; NaN or
// infinity counts as 0
__device__ __forceinline__ double face_norm(const float* __restrict__ points, const int* __restrict__ fv, int f, int V) {
#pragma clang fp contract(off)
  const size_t ia = 3 * (size_t)clampi(fv[3 * (size_t)f], V), ib = 3 * (size_t)clampi(fv[3 * (size_t)f + 1], V),
               ic = 3 * (size_t)clampi(fv[3 * (size_t)f + 2], V);
  const double ax = points[ia], ay = points[ia + 1], az = points[ia + 2];
  const double e1x = (double)points[ib] - ax, e1y = (double)points[ib + 1] - ay, e1z = (double)points[ib + 2] - az;
  const double e2x = (double)points[ic] - ax, e2y = (double)points[ic + 1] - ay, e2z = (double)points[ic + 2] - az;
  const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
  const double v = sqrt((cx * cx + cy * cy) + cz * cz);
  return v <= 1.7976931348623157e308 ? v : 0.0;
}

__global__ __launch_bounds__(kThreads) void face_norm_kernel(const float* __restrict__ points, const int* __restrict__ fv,
                                                             int F, int V, double* __restrict__ d,
                                                             double* __restrict__ partial) {
  double m = 0.0;
  for (int f = blockIdx.x * kThreads + threadIdx.x; f < F; f += gridDim.x * kThreads) {
    const double v = face_norm(points, fv, f, V);
    d[f] = v;
    m = fmax(m, v);
  }
  m = block_max_fp64(m);
  if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// one block: dmax over the blocks' maxima -> exponent[0]
__global__ __launch_bounds__(kThreads) void face_exponent_kernel(const double* __restrict__ partial, int n,
                                                                 int* __restrict__ exponent) {
  double m = 0.0;
  for (int b = threadIdx.x; b < n; b += kThreads) m = fmax(m, partial[b]);
  m = block_max_fp64(m);
  if (threadIdx.x == 0) {
    int e = 0;
    (void)frexp(m, &e);
    exponent[0] = m > 0.0 ? e : 0;
  }
}

__global__ __launch_bounds__(kThreads) void face_weight_kernel(const double* __restrict__ d, int F,
                                                               const int* __restrict__ exponent,
                                                               long long* __restrict__ weight) {
  const int shift = 32 - exponent[0];
  for (int f = blockIdx.x * kThreads + threadIdx.x; f < F; f += gridDim.x * kThreads)
    weight[f] = (long long)floor(ldexp(d[f], shift));      // d < 2^e: below 2^32
}

// ---- union batch: blocks per part.  block_begin[k] is the first workgroup of part k of this launch, one workgroup per
// kThreads faces (no grid stride); the launcher hands every launch its own stretch of `partial`, one maximum per workgroup.
struct WeightPartsJob {
  PartTable<int> f;                     // face rows of part k
  int block_begin[kMaxParts + 1];
};

__global__ __launch_bounds__(kThreads) void face_norm_parts_kernel(WeightPartsJob job, const float* __restrict__ points,
                                                                   const int* __restrict__ fv, int V,
                                                                   double* __restrict__ d, double* __restrict__ partial) {
  int p = 0;
  while (p + 1 < job.f.n && (int)blockIdx.x >= job.block_begin[p + 1]) ++p;    // wave-uniform
  const int f = job.f.begin[p] + ((int)blockIdx.x - job.block_begin[p]) * kThreads + (int)threadIdx.x;
  double v = 0.0;
  if (f < job.f.begin[p + 1]) {
    v = face_norm(points, fv, f, V);
    d[f] = v;
  }
  const double m = block_max_fp64(v);
  if (threadIdx.x == 0) partial[blockIdx.x] = m;
}

// one block per part: dmax over the part's workgroups -> exponent[part]
__global__ __launch_bounds__(kThreads) void face_exponent_parts_kernel(WeightPartsJob job, const double* __restrict__ partial,
                                                                       int* __restrict__ exponent) {
  const int p = blockIdx.x;
  double m = 0.0;
  for (int b = job.block_begin[p] + (int)threadIdx.x; b < job.block_begin[p + 1]; b += kThreads) m = fmax(m, partial[b]);
  m = block_max_fp64(m);
  if (threadIdx.x == 0) {
    int e = 0;
    (void)frexp(m, &e);
    exponent[p] = m > 0.0 ? e : 0;
  }
}

__global__ __launch_bounds__(kThreads) void face_weight_parts_kernel(PartTable<int> tab, const double* __restrict__ d,
                                                                     const int* __restrict__ exponent,
                                                                     long long* __restrict__ weight) {
  __shared__ int s_f[kMaxParts + 1];
  stage_parts(s_f, tab);
  __syncthreads();
  const int f = s_f[0] + blockIdx.x * kThreads + threadIdx.x;
  if (f >= s_f[tab.n]) return;
  weight[f] = (long long)floor(ldexp(d[f], 32 - exponent[find_part(s_f, tab.n, f)]));      // d < 2^e: below 2^32
}

// cum[f] = scan[f] - scan[first row of f's part - 1]: the part's own inclusive scan (integers: exact)
__global__ __launch_bounds__(kThreads) void part_cum_kernel(PartTable<int> tab, const long long* __restrict__ scan,
                                                            long long* __restrict__ cum) {
  __shared__ int s_f[kMaxParts + 1];
  stage_parts(s_f, tab);
  __syncthreads();
  const int f = s_f[0] + blockIdx.x * kThreads + threadIdx.x;
  if (f >= s_f[tab.n]) return;
  const int b = s_f[find_part(s_f, tab.n, f)];
  cum[f] = scan[f] - (b > 0 ? scan[b - 1] : 0ll);
}

// entry k of the table is cum[table_pos(k, F)]; the last entry is cum[F - 1].  F > kTable: strictly increasing from >= 0.
__device__ __forceinline__ int table_pos(int k, int F) { return (int)(((long long)(k + 1) * F) / kTable) - 1; }

// THE draw: rows i = block * kThreads + tid, stride blocks * kThreads, of N samples from a mesh of F faces whose rows in fv
// / cum start at the pointers given; out_face[i] = the face row + face_base.  The whole workgroup runs it together.
__device__ __forceinline__ void draw_rows(const float* __restrict__ points, const int* __restrict__ fv,
                                          const unsigned long long* __restrict__ cum, int F, int V, int N, uint32_t first,
                                          uint32_t k0, uint32_t k1, uint32_t stream_id, uint32_t draw, int face_base,
                                          int block, int blocks, float* __restrict__ out_points,
                                          int* __restrict__ out_face, float* __restrict__ out_bary) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_tab[kTable];
  const bool whole = F <= kTable;                   // all of cum sits in the table
  const int n_tab = whole ? F : kTable;
  for (int k = threadIdx.x; k < n_tab; k += kThreads) s_tab[k] = cum[whole ? k : table_pos(k, F)];
  __syncthreads();
  const unsigned long long total = s_tab[n_tab - 1];
  for (int i = block * kThreads + threadIdx.x; i < N; i += blocks * kThreads) {
    const size_t o = 3 * (size_t)i;
    if (total == 0) {
      out_face[i] = -1;
      out_points[o] = out_points[o + 1] = out_points[o + 2] = 0.f;
      out_bary[o] = out_bary[o + 1] = out_bary[o + 2] = 0.f;
      continue;
    }
    const U4 w = philox4x32_10(first + (uint32_t)i, stream_id, draw, 2u, k0, k1);
    const unsigned long long r = (unsigned long long)w.x << 32 | w.y;
    const unsigned long long t = __umul64hi(r, total);     // < total = the last entry: the searches below always end
    int lo = 0, hi = n_tab - 1;                            // first table entry > t
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_tab[mid] > t) hi = mid; else lo = mid + 1;
    }
    int face = lo;
    if (!whole) {                                          // cum[pos(lo - 1)] <= t < cum[pos(lo)]: finish inside the bucket
      int a = lo == 0 ? 0 : table_pos(lo - 1, F) + 1, b = table_pos(lo, F);
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (cum[mid] > t) b = mid; else a = mid + 1;
      }
      face = a;
    }
    float u1 = word_uniform(w.z), u2 = word_uniform(w.w);
    if (u1 + u2 > 1.0f) {
      u1 = 1.0f - u1;
      u2 = 1.0f - u2;
    }
    const float b0 = (1.0f - u1) - u2;
    const size_t ia = 3 * (size_t)clampi(fv[3 * (size_t)face], V), ib = 3 * (size_t)clampi(fv[3 * (size_t)face + 1], V),
                 ic = 3 * (size_t)clampi(fv[3 * (size_t)face + 2], V);
    out_face[i] = face_base + face;
    out_bary[o] = b0;
    out_bary[o + 1] = u1;
    out_bary[o + 2] = u2;
    for (int k = 0; k < 3; ++k) out_points[o + k] = fmaf(u2, points[ic + k], fmaf(u1, points[ib + k], b0 * points[ia + k]));
  }
}

__global__ __launch_bounds__(kThreads) void sample_surface_kernel(
    const float* __restrict__ points, const int* __restrict__ fv, const unsigned long long* __restrict__ cum, int F, int V,
    int N, uint32_t first, uint32_t k0, uint32_t k1, uint32_t stream_id, uint32_t draw, float* __restrict__ out_points,
    int* __restrict__ out_face, float* __restrict__ out_bary) {
  draw_rows(points, fv, cum, F, V, N, first, k0, k1, stream_id, draw, 0, blockIdx.x, gridDim.x, out_points, out_face,
            out_bary);
}

// union batch: part k of the launch owns the workgroups k * blocks_per_part .. and the output rows (row0 + k) * N ..
struct DrawPartsJob {
  PartTable<int> f;                     // face rows of part k
  uint32_t stream_id[kMaxParts];
};

__global__ __launch_bounds__(kThreads) void sample_surface_parts_kernel(
    DrawPartsJob job, int blocks_per_part, int row0, const float* __restrict__ points, const int* __restrict__ fv,
    const unsigned long long* __restrict__ cum, int V, int N, uint32_t first, uint32_t k0, uint32_t k1, uint32_t draw,
    float* __restrict__ out_points, int* __restrict__ out_face, float* __restrict__ out_bary) {
  const int p = (int)blockIdx.x / blocks_per_part;                             // wave-uniform, < job.f.n by the grid
  const int f0 = job.f.begin[p];
  const size_t o = (size_t)(row0 + p) * (size_t)N;
  draw_rows(points, fv + 3 * (size_t)f0, cum + f0, job.f.begin[p + 1] - f0, V, N, first, k0, k1, job.stream_id[p], draw, f0,
            (int)blockIdx.x - p * blocks_per_part, blocks_per_part, out_points + 3 * o, out_face + o, out_bary + 3 * o);
}

struct WeightBuffers {
  double *d, *partial;
  InclusiveScan<long long> scan;
};
WeightBuffers carve_weights(Arena& a, int64_t F) {
  return {a.take<double>(F), a.take<double>(kMaxBlocks), InclusiveScan<long long>::take(a, F)};
}

struct WeightPartsBuffers {
  double *d, *partial;
  long long* scan;
  InclusiveScan<long long> scan_step;
};
// partial: one maximum per workgroup, at most F / kThreads + P of them
WeightPartsBuffers carve_weights_parts(Arena& a, int64_t F, int P) {
  return {a.take<double>(F), a.take<double>(F / kThreads + P), a.take<long long>(F),
          InclusiveScan<long long>::take(a, F)};
}

// the face pointer of a union batch: parts_check, and it starts at row 0
int face_parts_check(const char* fn, const int64_t* fptr, int P) {
  GEOBI_TRY(parts_check(fn, fptr, fptr, P));
  GEOBI_REQUIRE(fptr[0] == 0, "%s: fptr starts at %lld (it cuts the rows of fv: 0)", fn, (long long)fptr[0]);
  return 0;
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

int geobi_sample_table_entries(void) { return kTable; }

size_t geobi_sample_ws_bytes(int64_t F) {
  return F < 1 || F > GEOBI_MAX_NODES ? 0 : carve_bytes([&](Arena& a) { carve_weights(a, F); });
}

int geobi_sample_weights(const float* points, const int32_t* fv, int64_t F, int64_t V, void* weight, void* cum,
                         int32_t* exponent, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(F > V ? F : V, 0);
  GEOBI_REQUIRE(F >= 1 && V >= 1, "%s: F = %lld faces, V = %lld vertices (at least one of each)", __func__, (long long)F,
                (long long)V);
  GEOBI_NOTNULL(points); GEOBI_NOTNULL(fv); GEOBI_NOTNULL(weight); GEOBI_NOTNULL(cum); GEOBI_NOTNULL(exponent);
  GEOBI_NOTNULL(ws);
  hipStream_t s = as_stream(stream);
  Arena a(ws, ws_bytes);
  const WeightBuffers w = carve_weights(a, F);
  GEOBI_WS_CHECK("sample_weights", a, ws, ws_bytes);
  int blocks = cdiv(F, kThreads);
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  face_norm_kernel<<<blocks, kThreads, 0, s>>>(points, fv, (int)F, (int)V, w.d, w.partial);
  GEOBI_LAUNCH_OK();
  face_exponent_kernel<<<1, kThreads, 0, s>>>(w.partial, blocks, exponent);
  GEOBI_LAUNCH_OK();
  face_weight_kernel<<<blocks, kThreads, 0, s>>>(w.d, (int)F, exponent, (long long*)weight);
  GEOBI_LAUNCH_OK();
  return w.scan.run((long long*)weight, (long long*)cum, s);
}

int geobi_sample_surface(const float* points, const int32_t* fv, const void* cum, int64_t F, int64_t V, int64_t N,
                         int64_t first, uint64_t seed, uint32_t stream_id, uint32_t draw, float* out_points,
                         int32_t* out_face, float* out_bary, void* stream) {
  GEOBI_SIZES(F > V ? F : V, 0);
  GEOBI_SIZES(N, 0);
  GEOBI_REQUIRE(first >= 0 && first + N <= GEOBI_MAX_NODES, "%s: first = %lld, first + N = %lld outside [0, GEOBI_MAX_NODES = %d]",
                __func__, (long long)first, (long long)(first + N), GEOBI_MAX_NODES);
  GEOBI_REQUIRE(F >= 1 && V >= 1, "%s: F = %lld faces, V = %lld vertices (at least one of each)", __func__, (long long)F,
                (long long)V);
  if (N == 0) return 0;
  GEOBI_NOTNULL(points); GEOBI_NOTNULL(fv); GEOBI_NOTNULL(cum); GEOBI_NOTNULL(out_points); GEOBI_NOTNULL(out_face);
  GEOBI_NOTNULL(out_bary);
  hipStream_t s = as_stream(stream);
  if (N == 0) return 0;
  int blocks = cdiv(N, kThreads);
  if (blocks > kMaxBlocks) blocks = kMaxBlocks;
  sample_surface_kernel<<<blocks, kThreads, 0, s>>>(points, fv, (const unsigned long long*)cum, (int)F, (int)V, (int)N,
                                                    (uint32_t)first, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32),
                                                    stream_id, draw, out_points, out_face, out_bary);
  GEOBI_LAUNCH_OK();
  return 0;
}

size_t geobi_sample_parts_ws_bytes(int64_t F, int P) {
  return F < 1 || F > GEOBI_MAX_NODES || P < 1 || P > F ? 0 : carve_bytes([&](Arena& a) { carve_weights_parts(a, F, P); });
}

int geobi_sample_weights_parts(const float* points, const int32_t* fv, const int64_t* fptr, int P, int64_t V, void* weight,
                               void* cum, int32_t* exponent, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_TRY(face_parts_check(__func__, fptr, P));
  GEOBI_SIZES(V, 0);
  GEOBI_REQUIRE(V >= 1, "%s: V = %lld vertices (at least one)", __func__, (long long)V);
  GEOBI_NOTNULL(points); GEOBI_NOTNULL(fv); GEOBI_NOTNULL(weight); GEOBI_NOTNULL(cum); GEOBI_NOTNULL(exponent);
  GEOBI_NOTNULL(ws);
  hipStream_t s = as_stream(stream);
  const int64_t F = fptr[P];
  Arena a(ws, ws_bytes);
  const WeightPartsBuffers w = carve_weights_parts(a, F, P);
  GEOBI_WS_CHECK("sample_weights_parts", a, ws, ws_bytes);
  int used = 0;                                          // workgroups so far = entries of `partial`
  for (int base = 0; base < P; base += kMaxParts) {
    WeightPartsJob job;
    fill_parts(&job.f, fptr, base, P);
    int blocks = 0;
    for (int k = 0; k <= kMaxParts; ++k) {               // the unused tail: no blocks
      job.block_begin[k] = blocks;
      if (k < job.f.n) blocks += cdiv(job.f.begin[k + 1] - job.f.begin[k], kThreads);
    }
    const int rows = job.f.begin[job.f.n] - job.f.begin[0];
    face_norm_parts_kernel<<<blocks, kThreads, 0, s>>>(job, points, fv, (int)V, w.d, w.partial + used);
    face_exponent_parts_kernel<<<job.f.n, kThreads, 0, s>>>(job, w.partial + used, exponent + base);
    face_weight_parts_kernel<<<cdiv(rows, kThreads), kThreads, 0, s>>>(job.f, w.d, exponent + base, (long long*)weight);
    GEOBI_LAUNCH_OK();
    used += blocks;
  }
  GEOBI_TRY(w.scan_step.run((long long*)weight, w.scan, s));
  for (int base = 0; base < P; base += kMaxParts) {
    PartTable<int> tab;
    fill_parts(&tab, fptr, base, P);
    part_cum_kernel<<<cdiv(tab.begin[tab.n] - tab.begin[0], kThreads), kThreads, 0, s>>>(tab, w.scan, (long long*)cum);
  }
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_sample_surface_parts(const float* points, const int32_t* fv, const void* cum, const int64_t* fptr, int P, int64_t V,
                               int64_t N, int64_t first, uint64_t seed, const uint32_t* stream_id, uint32_t draw,
                               float* out_points, int32_t* out_face, float* out_bary, void* stream) {
  GEOBI_TRY(face_parts_check(__func__, fptr, P));
  GEOBI_SIZES(V, 0);
  GEOBI_SIZES(N, 0);
  GEOBI_REQUIRE(V >= 1, "%s: V = %lld vertices (at least one)", __func__, (long long)V);
  GEOBI_REQUIRE((int64_t)P * N <= GEOBI_MAX_NODES, "%s: P * N = %lld rows exceed GEOBI_MAX_NODES = %d", __func__,
                (long long)((int64_t)P * N), GEOBI_MAX_NODES);
  GEOBI_REQUIRE(first >= 0 && first + N <= GEOBI_MAX_NODES, "%s: first = %lld, first + N = %lld outside [0, GEOBI_MAX_NODES = %d]",
                __func__, (long long)first, (long long)(first + N), GEOBI_MAX_NODES);
  GEOBI_NOTNULL(stream_id);
  if (N == 0) return 0;
  GEOBI_NOTNULL(points); GEOBI_NOTNULL(fv); GEOBI_NOTNULL(cum); GEOBI_NOTNULL(out_points); GEOBI_NOTNULL(out_face);
  GEOBI_NOTNULL(out_bary);
  hipStream_t s = as_stream(stream);
  int per_part = cdiv(N, kThreads);                      // the single-mesh grid, per part
  if (per_part > kMaxBlocks) per_part = kMaxBlocks;
  for (int base = 0; base < P; base += kMaxParts) {
    DrawPartsJob job;
    fill_parts(&job.f, fptr, base, P);
    for (int k = 0; k < kMaxParts; ++k) job.stream_id[k] = k < job.f.n ? stream_id[base + k] : 0u;
    sample_surface_parts_kernel<<<job.f.n * per_part, kThreads, 0, s>>>(
        job, per_part, base, points, fv, (const unsigned long long*)cum, (int)V, (int)N, (uint32_t)first,
        (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), draw, out_points, out_face, out_bary);
  }
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
