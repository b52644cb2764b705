// Brute-force nearest distances between point sets and from points to a triangle mesh: the vertex metric of the
// denoising evaluation.
//
//   nearest_point     code/data_util.py:604 (my_hausdorff.nearest_distance, numba prange on the CPU)
//   nearest_triangle  data_util.py:601-603 (the commented-out p2m: point-to-surface distance)
//   dist_summary      the .sum() / .mean() / max over the per-vertex distances, data_util.py:610-616
//   nearest_parts     nearest_point confined to the meshes of a union batch: the search under the correspondence-free
//                     losses, code/network.py:369-370 (chamfer_distance) and :385-388 (sided_distance)
//
// ONE all-pairs walk (nearest_walk) serves the three searches: a lane owns QPL queries in registers; the workgroup
// stages a tile of targets in LDS (for triangles: a 16-float record per triangle, corners gathered once per tile); every
// lane walks the tile reading the SAME address (LDS broadcast, no bank conflict), so one LDS record feeds QPL pair
// tests.  What differs between points and triangles is a target policy (PointTargets, TriangleTargets: tile size, LDS
// record, staging, pair test); what differs between the single-mesh and the per-part search is where the kernel takes
// the row ranges q0, q_end, t_begin, t_end from.  So for any part the answer is what nearest_point gives on that part's
// rows alone: it is the same text.
//
// Determinism: the target set is cut into S slices of whole tiles so that a small query set still fills the chip
// (slice_targets: the one slicing rule); a (query block, slice) workgroup writes per query its partial (d2, index) and
// nearest_reduce_kernel reduces the S partials in ascending slice order.  Comparisons are strict (<) in ascending
// target order at both stages, so ties go to the LOWEST index, and since min is exact and a pair's d2 is formed by the
// same instruction sequence whatever the slicing (contraction is off in the pair functions; every fused multiply-add is
// written out), the result is bit-identical for every S.  d2 is formed from coordinate DIFFERENCES, never
// |q|^2 + |t|^2 - 2 q.t; one sqrt per query at the end.
#include "common.h"
#include "dist_pairs.h"
#include "pair_slices.h"
#include "../../include/geobi_hip.h"

#include <math.h>

#include <algorithm>
#include <type_traits>

namespace geobi {

namespace {

constexpr int kThreads = 256;
#ifndef GEOBI_DIST_POINT_TILE
#define GEOBI_DIST_POINT_TILE 512                   // 512 beat 1024 and 256 (profiles/mesheval_kernels.txt); A/B: tools/build_variant.sh
#endif
constexpr int kPointQpl = 4, kPointTile = GEOBI_DIST_POINT_TILE;     // LDS: float4 per target point
constexpr int kTriQpl = 2, kTriTile = 256;          // 16 KB of LDS: four float4 per triangle
static_assert(kThreads == kWalkThreads, "the slicing rule (pair_slices.h) counts query blocks of kWalkThreads lanes");

// ---------------------------------------------------------------- the walk
// Queries q0 .. q_end of this workgroup (QPL per lane, kThreads apart) against targets t_begin .. t_end; the partial
// (d2, index) of query i goes to part_*[slice * ld_part + i].  Tail lanes repeat the range's last query and write
// nothing.  bidx starts at t_begin: in range whatever the coordinates are (a NaN query never passes the <).
template <class Targets>
__device__ __forceinline__ void nearest_walk(const Targets& tg, const float* __restrict__ q, int q0, int q_end, int t_begin,
                                             int t_end, int slice, int ld_part, float* __restrict__ part_d2,
                                             int* __restrict__ part_idx) {
  constexpr int kQpl = Targets::kQpl, kTile = Targets::kTile;
  __shared__ typename Targets::Tile tile;
  const int tid = threadIdx.x;
  float qx[kQpl], qy[kQpl], qz[kQpl], best[kQpl];
  int bidx[kQpl];
#pragma unroll
  for (int k = 0; k < kQpl; ++k) {
    const int i = min(q0 + k * kThreads + tid, q_end - 1);
    qx[k] = q[3 * (size_t)i]; qy[k] = q[3 * (size_t)i + 1]; qz[k] = q[3 * (size_t)i + 2];
    best[k] = INFINITY;
    bidx[k] = t_begin;
  }
  for (int t0 = t_begin; t0 < t_end; t0 += kTile) {
    const int n = min(kTile, t_end - t0);
    __syncthreads();
    tg.stage(tile, t0, n, tid);
    __syncthreads();
#pragma unroll Targets::kUnroll
    for (int j = 0; j < n; ++j) {
      const typename Targets::Record r = Targets::load(tile, j);
#pragma unroll
      for (int k = 0; k < kQpl; ++k) {
        const float d2 = Targets::d2(qx[k], qy[k], qz[k], r);
        const bool lt = d2 < best[k];
        best[k] = lt ? d2 : best[k];
        bidx[k] = lt ? t0 + j : bidx[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kQpl; ++k) {
    const int i = q0 + k * kThreads + tid;
    if (i < q_end) {
      part_d2[(size_t)slice * ld_part + i] = best[k];
      part_idx[(size_t)slice * ld_part + i] = bidx[k];
    }
  }
}

// ---------------------------------------------------------------- point - point
struct PointTargets {                               // LDS: one float4 per target point
  static constexpr int kQpl = kPointQpl, kTile = kPointTile, kUnroll = 4;
  struct Tile { float4 p[kTile]; };
  using Record = float4;
  const float* __restrict__ t;
  __device__ __forceinline__ void stage(Tile& tile, int t0, int n, int tid) const {
    for (int j = tid; j < n; j += kThreads) {
      const float* p = t + 3 * (size_t)(t0 + j);
      tile.p[j] = make_float4(p[0], p[1], p[2], 0.f);
    }
  }
  static __device__ __forceinline__ Record load(const Tile& tile, int j) { return tile.p[j]; }
  static __device__ __forceinline__ float d2(float qx, float qy, float qz, const Record& r) { return pair_d2(qx, qy, qz, r); }
};

__global__ __launch_bounds__(kThreads) void nearest_point_kernel(const float* __restrict__ q, const float* __restrict__ t,
                                                                 int Q, int T, int tiles_per_slice,
                                                                 float* __restrict__ part_d2, int* __restrict__ part_idx) {
  const int slice = blockIdx.y;
  const int t_begin = slice * tiles_per_slice * kPointTile;
  nearest_walk(PointTargets{t}, q, blockIdx.x * (kThreads * kPointQpl), Q, t_begin,
               min(T, t_begin + tiles_per_slice * kPointTile), slice, Q, part_d2, part_idx);
}

// The same search confined to the parts of a disjoint-union batch (code/network.py:369-370 chamfer_distance, :385-388
// sided_distance): queries of part p only meet targets of part p.  A workgroup belongs to ONE part (blocks are formed
// per part); the part tables ride in the kernel arguments (common.h).
struct PartsJob {
  PartTable<int> q, t;                  // query / target rows of part k
  int block_begin[kMaxParts + 1];       // first workgroup (blockIdx.x) of part k
  int tiles_per_slice[kMaxParts];
  int slices[kMaxParts];                // >= 1, no empty slice
};

__global__ __launch_bounds__(kThreads) void nearest_parts_kernel(PartsJob job, const float* __restrict__ q,
                                                                 const float* __restrict__ t, int ld_part,
                                                                 float* __restrict__ part_d2, int* __restrict__ part_idx) {
  int p = 0;
  while (p + 1 < job.q.n && (int)blockIdx.x >= job.block_begin[p + 1]) ++p;    // wave-uniform
  const int slice = blockIdx.y;
  if (slice >= job.slices[p]) return;                                         // the whole workgroup leaves together
  const int span = job.tiles_per_slice[p] * kPointTile;
  const int t_begin = job.t.begin[p] + slice * span;
  nearest_walk(PointTargets{t}, q, job.q.begin[p] + ((int)blockIdx.x - job.block_begin[p]) * (kThreads * kPointQpl),
               job.q.begin[p + 1], t_begin, min(job.t.begin[p + 1], t_begin + span), slice, ld_part, part_d2, part_idx);
}

// The partials of a query's slices in ascending order, strict <: the lowest index among equal distances survives.
// OneRange: rows 0 .. rows with S slices each, the distance (sqrt) goes out and idx may be NULL; PartsJob: a query
// has the slice count of its own part and the SQUARED distance goes out.
struct OneRange { int rows, slices; };

template <class Job>
__global__ __launch_bounds__(kThreads) void nearest_reduce_kernel(Job job, const float* __restrict__ part_d2,
                                                                  const int* __restrict__ part_idx, int ld_part,
                                                                  float* __restrict__ out, int* __restrict__ idx) {
  constexpr bool kParts = std::is_same<Job, PartsJob>::value;
  int i = blockIdx.x * kThreads + threadIdx.x, S;
  if constexpr (kParts) {
    __shared__ int s_begin[kMaxParts + 1], s_slices[kMaxParts];
    stage_parts(s_begin, job.q);
    for (int k = threadIdx.x; k < job.q.n; k += kThreads) s_slices[k] = job.slices[k];
    __syncthreads();
    i += s_begin[0];
    if (i >= s_begin[job.q.n]) return;
    S = s_slices[find_part(s_begin, job.q.n, i)];
  } else {
    if (i >= job.rows) return;
    S = job.slices;
  }
  float best = part_d2[i];
  int b = part_idx[i];
  for (int s = 1; s < S; ++s) {
    const float d2 = part_d2[(size_t)s * ld_part + i];
    const int j = part_idx[(size_t)s * ld_part + i];
    if (d2 < best) { best = d2; b = j; }
  }
  out[i] = kParts ? best : sqrtf(best);
  if (kParts || idx) idx[i] = b;
}

// ---------------------------------------------------------------- point - triangle
// pair functions and the record of a triangle: dist_pairs.h

struct TriangleTargets {                            // 16 KB of LDS: four float4 per triangle
  static constexpr int kQpl = kTriQpl, kTile = kTriTile, kUnroll = 2;
  static_assert(kTile == kThreads, "one thread stages one triangle of the tile");
  struct Tile { float4 r[4][kTile]; };
  struct Record { float4 r0, r1, r2, r3; };
  const float* __restrict__ verts;
  const int* __restrict__ fv;
  int V;
  __device__ __forceinline__ void stage(Tile& tile, int f0, int n, int tid) const {
    if (tid < n) triangle_record(verts, fv, V, f0 + tid, &tile.r[0][tid], &tile.r[1][tid], &tile.r[2][tid], &tile.r[3][tid]);
  }
  static __device__ __forceinline__ Record load(const Tile& tile, int j) {
    return {tile.r[0][j], tile.r[1][j], tile.r[2][j], tile.r[3][j]};
  }
  static __device__ __forceinline__ float d2(float qx, float qy, float qz, const Record& r) {
    return tri_d2(qx, qy, qz, r.r0, r.r1, r.r2, r.r3);
  }
};

__global__ __launch_bounds__(kThreads) void nearest_triangle_kernel(const float* __restrict__ q,
                                                                    const float* __restrict__ verts,
                                                                    const int* __restrict__ fv, int Q, int V, int F,
                                                                    int tiles_per_slice, float* __restrict__ part_d2,
                                                                    int* __restrict__ part_idx) {
  const int slice = blockIdx.y;
  const int f_begin = slice * tiles_per_slice * kTriTile;
  nearest_walk(TriangleTargets{verts, fv, V}, q, blockIdx.x * (kThreads * kTriQpl), Q, f_begin,
               min(F, f_begin + tiles_per_slice * kTriTile), slice, Q, part_d2, part_idx);
}

// ---------------------------------------------------------------- sum / max of a distance vector
// fp64 accumulation, fixed order: thread-strided partial sums, block_sum_fp64, the blocks in ascending order.
__global__ __launch_bounds__(kThreads) void dist_summary_partial_kernel(const float* __restrict__ d, int64_t n,
                                                                        double* __restrict__ partial) {
  __shared__ float smax[kThreads];
  double s = 0.0;
  float m = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const float x = d[i];
    s += (double)x;
    m = fmaxf(m, x);
  }
  smax[threadIdx.x] = m;
  const double sum = block_sum_fp64<kThreads>(s, [&](int h) { smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + h]); });
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = sum;
    partial[2 * blockIdx.x + 1] = (double)smax[0];
  }
}

__global__ void dist_summary_final_kernel(const double* __restrict__ partial, int blocks, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double m = -INFINITY;
  for (int b = 0; b < blocks; ++b) m = fmax(m, partial[2 * b + 1]);
  out[0] = fold_ascending(partial, blocks, 2);
  out[1] = m;
}

int summary_blocks(int64_t n) {
  const int64_t b = (n + 4 * kThreads - 1) / (4 * kThreads);
  return (int)(b < 1 ? 1 : (b > 512 ? 512 : b));
}

// per slice and query row: the best squared distance and its target
struct Partials { float* d2; int* idx; };
Partials carve_partials(Arena& a, int slices, int64_t rows) {
  return {a.take<float>((size_t)slices * rows), a.take<int>((size_t)slices * rows)};
}
size_t partials_bytes(int slices, int64_t rows) { return carve_bytes([&](Arena& a) { carve_partials(a, slices, rows); }); }
double* carve_summary(Arena& a, int blocks) { return a.take<double>((size_t)2 * blocks); }

// every part is sliced as a single mesh would be, but for the workgroups of ALL parts together (P = 1: choose_slices)
int parts_want(const int64_t* qptr, int P) {
  int64_t qblocks = 0;
  for (int p = 0; p < P; ++p) qblocks += cdiv(qptr[p + 1] - qptr[p], (int64_t)kThreads * kPointQpl);
  return want_slices(qblocks);
}
Slicing part_slices(const int64_t* qptr, const int64_t* tptr, int p, int want) {
  return slice_targets(qptr[p + 1] - qptr[p], tptr[p + 1] - tptr[p], kPointQpl, kPointTile, want);
}
int max_part_slices(const int64_t* qptr, const int64_t* tptr, int P) {
  const int want = parts_want(qptr, P);
  int smax = 0;
  for (int p = 0; p < P; ++p) smax = std::max(smax, part_slices(qptr, tptr, p, want).slices);
  return smax;
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

int geobi_nearest_slices(int64_t Q, int64_t T, int triangles) {
  if (Q <= 0 || T <= 0) return 0;
  return triangles ? choose_slices(Q, T, kTriQpl, kTriTile).slices : choose_slices(Q, T, kPointQpl, kPointTile).slices;
}

size_t geobi_nearest_ws_bytes(int64_t Q, int64_t T) {
  if (Q <= 0 || T <= 0) return partials_bytes(0, 0);
  // enough for either kernel
  return std::max(partials_bytes(choose_slices(Q, T, kPointQpl, kPointTile).slices, Q),
                  partials_bytes(choose_slices(Q, T, kTriQpl, kTriTile).slices, Q));
}

int geobi_nearest_point(const float* q, const float* t, int64_t Q, int64_t T, float* dist, int32_t* idx, void* ws,
                        size_t ws_bytes, void* stream) {
  GEOBI_SIZES(Q > T ? Q : T, 0);
  GEOBI_NOTNULL(q); GEOBI_NOTNULL(t); GEOBI_NOTNULL(dist); GEOBI_NOTNULL(ws);
  GEOBI_REQUIRE(Q > 0 && T > 0, "nearest_point: empty query or target set (Q = %lld, T = %lld)", (long long)Q, (long long)T);
  hipStream_t s = as_stream(stream);
  const Slicing c = choose_slices(Q, T, kPointQpl, kPointTile);
  Arena ar(ws, ws_bytes);
  const Partials p = carve_partials(ar, c.slices, Q);
  GEOBI_WS_CHECK("nearest_point", ar, ws, ws_bytes);
  nearest_point_kernel<<<dim3(c.qblocks, c.slices), kThreads, 0, s>>>(q, t, (int)Q, (int)T, c.tiles_per_slice, p.d2, p.idx);
  nearest_reduce_kernel<<<cdiv(Q, kThreads), kThreads, 0, s>>>(OneRange{(int)Q, c.slices}, p.d2, p.idx, (int)Q, dist, idx);
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_nearest_parts_slices(const int64_t* qptr, const int64_t* tptr, int P) {
  return parts_check("nearest_parts_slices", qptr, tptr, P) == 0 ? max_part_slices(qptr, tptr, P) : 0;
}

size_t geobi_nearest_parts_ws_bytes(const int64_t* qptr, const int64_t* tptr, int P) {
  const int smax = geobi_nearest_parts_slices(qptr, tptr, P);      // 0: the part pointers failed their check
  return partials_bytes(smax, smax == 0 ? 0 : qptr[P]);
}

int geobi_nearest_parts(const float* q, const float* t, const int64_t* qptr, const int64_t* tptr, int P, float* d2,
                        int32_t* idx, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_TRY(parts_check(__func__, qptr, tptr, P));
  GEOBI_NOTNULL(q); GEOBI_NOTNULL(t); GEOBI_NOTNULL(d2); GEOBI_NOTNULL(idx); GEOBI_NOTNULL(ws);
  hipStream_t s = as_stream(stream);
  const int want = parts_want(qptr, P);
  const int smax = max_part_slices(qptr, tptr, P);
  const int ld = (int)qptr[P];
  Arena ar(ws, ws_bytes);
  const Partials p = carve_partials(ar, smax, ld);
  GEOBI_WS_CHECK("nearest_parts", ar, ws, ws_bytes);
  for (int base = 0; base < P; base += kMaxParts) {
    PartsJob job;
    fill_parts(&job.q, qptr, base, P);
    fill_parts(&job.t, tptr, base, P);
    int blocks = 0, sl_max = 0;
    for (int k = 0; k <= kMaxParts; ++k) {                // the unused tail: no blocks, one slice
      const Slicing c = k < job.q.n ? part_slices(qptr, tptr, base + k, want) : Slicing{0, 1, 1};
      job.block_begin[k] = blocks;
      if (k < kMaxParts) { job.tiles_per_slice[k] = c.tiles_per_slice; job.slices[k] = c.slices; }
      blocks += c.qblocks;
      if (k < job.q.n) sl_max = std::max(sl_max, c.slices);
    }
    nearest_parts_kernel<<<dim3(blocks, sl_max), kThreads, 0, s>>>(job, q, t, ld, p.d2, p.idx);
    const int rows = job.q.begin[job.q.n] - job.q.begin[0];
    nearest_reduce_kernel<<<cdiv(rows, kThreads), kThreads, 0, s>>>(job, p.d2, p.idx, ld, d2, idx);
  }
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_nearest_triangle(const float* q, const float* verts, const int32_t* fv, int64_t Q, int64_t V, int64_t F,
                           float* dist, int32_t* face, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(Q > V ? Q : V, 0);
  GEOBI_SIZES(F, 0);
  GEOBI_NOTNULL(q); GEOBI_NOTNULL(verts); GEOBI_NOTNULL(fv); GEOBI_NOTNULL(dist); GEOBI_NOTNULL(ws);
  GEOBI_REQUIRE(Q > 0 && V > 0 && F > 0, "nearest_triangle: empty query set or mesh (Q = %lld, V = %lld, F = %lld)",
                (long long)Q, (long long)V, (long long)F);
  hipStream_t s = as_stream(stream);
  const Slicing c = choose_slices(Q, F, kTriQpl, kTriTile);
  Arena ar(ws, ws_bytes);
  const Partials p = carve_partials(ar, c.slices, Q);
  GEOBI_WS_CHECK("nearest_triangle", ar, ws, ws_bytes);
  nearest_triangle_kernel<<<dim3(c.qblocks, c.slices), kThreads, 0, s>>>(q, verts, fv, (int)Q, (int)V, (int)F,
                                                                         c.tiles_per_slice, p.d2, p.idx);
  nearest_reduce_kernel<<<cdiv(Q, kThreads), kThreads, 0, s>>>(OneRange{(int)Q, c.slices}, p.d2, p.idx, (int)Q, dist, face);
  GEOBI_LAUNCH_OK();
  return 0;
}

size_t geobi_dist_summary_ws_bytes(int64_t n) { return carve_bytes([&](Arena& a) { carve_summary(a, summary_blocks(n)); }); }

int geobi_dist_summary(const float* dist, int64_t n, void* out, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_SIZES(n, 0);
  GEOBI_NOTNULL(dist); GEOBI_NOTNULL(out); GEOBI_NOTNULL(ws);
  GEOBI_REQUIRE(n > 0, "dist_summary: empty vector");
  hipStream_t s = as_stream(stream);
  Arena ar(ws, ws_bytes);
  const int blocks = summary_blocks(n);
  double* partial = carve_summary(ar, blocks);
  GEOBI_WS_CHECK("dist_summary", ar, ws, ws_bytes);
  dist_summary_partial_kernel<<<blocks, kThreads, 0, s>>>(dist, n, partial);
  dist_summary_final_kernel<<<1, 64, 0, s>>>(partial, blocks, (double*)out);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
