// Brute-force nearest distances between point sets and from points to a triangle mesh: the vertex metric of the
// denoising evaluation.
//
//   nearest_point     code/data_util.py:604 (my_hausdorff.nearest_distance, numba prange on the CPU)
//   nearest_triangle  data_util.py:601-603 (the commented-out p2m: point-to-surface distance)
//   dist_summary      the .sum() / .mean() / max over the per-vertex distances, data_util.py:610-616
//   nearest_parts     nearest_point confined to the meshes of a union batch: the search under the correspondence-free
//                     losses, code/network.py:369-370 (chamfer_distance) and :385-388 (sided_distance)
//
// Shape of the two all-pairs kernels: a lane owns QPL queries in registers; the workgroup stages a tile of targets
// in LDS (for triangles: a 16-float record per triangle, corners gathered once per tile); every lane walks the tile
// reading the SAME address (LDS broadcast, no bank conflict), so one 16-byte LDS read feeds QPL pair tests.
//
// Determinism: the target set is cut into S slices of whole tiles so that a small query set still fills the chip; a
// (query block, slice) workgroup writes per query its partial (d2, index) and a second kernel reduces the S partials in
// ascending slice order.  Comparisons are strict (<) in ascending target order at both stages, so ties go to the LOWEST
// index, and since min is exact and a pair's d2 is formed by the same instruction sequence whatever the slicing
// (contraction is off in the pair functions; every fused multiply-add is written out), the result is bit-identical
// for every S.  d2 is formed from coordinate DIFFERENCES, never |q|^2 + |t|^2 - 2 q.t; one sqrt per query at the end.
#include "common.h"

#include <math.h>

namespace geobi {

namespace {

constexpr int kThreads = 256;
#ifndef GEOBI_DIST_POINT_TILE
#define GEOBI_DIST_POINT_TILE 512                   // 512 beat 1024 and 256 (profiles/mesheval_kernels.txt); A/B: tools/build_variant.sh
#endif
constexpr int kPointQpl = 4, kPointTile = GEOBI_DIST_POINT_TILE;     // LDS: float4 per target point
constexpr int kTriQpl = 2, kTriTile = 256;          // 16 KB of LDS: four float4 per triangle
constexpr int kTargetBlocks = 1024;                 // workgroups wanted per launch (256 CUs x 4)
constexpr int kMaxSlices = 1024;

struct Slicing { int qblocks, slices, tiles_per_slice; };

Slicing choose_slices(int64_t Q, int64_t T, int qpl, int tile) {
  Slicing c;
  c.qblocks = cdiv(Q, (int64_t)kThreads * qpl);
  const int ntiles = cdiv(T, tile);
  int want = cdiv(kTargetBlocks, c.qblocks);
  if (want > kMaxSlices) want = kMaxSlices;
  if (want > ntiles) want = ntiles;
  if (want < 1) want = 1;
  c.tiles_per_slice = cdiv(ntiles, want);
  c.slices = cdiv(ntiles, c.tiles_per_slice);       // no empty slice
  return c;
}

// ---------------------------------------------------------------- point - point
__device__ __forceinline__ float pair_d2(float qx, float qy, float qz, float4 t) {
#pragma clang fp contract(off)
  const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
  return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}

__global__ __launch_bounds__(kThreads) void nearest_point_kernel(const float* __restrict__ q, const float* __restrict__ t,
                                                                 int Q, int T, int tiles_per_slice,
                                                                 float* __restrict__ part_d2, int* __restrict__ part_idx) {
  __shared__ float4 tile[kPointTile];
  const int tid = threadIdx.x;
  const int q0 = blockIdx.x * (kThreads * kPointQpl);
  const int slice = blockIdx.y;
  float qx[kPointQpl], qy[kPointQpl], qz[kPointQpl], best[kPointQpl];
  int bidx[kPointQpl];
  const int t_begin = slice * tiles_per_slice * kPointTile;
  const int t_end = min(T, t_begin + tiles_per_slice * kPointTile);
#pragma unroll
  for (int k = 0; k < kPointQpl; ++k) {
    const int i = min(q0 + k * kThreads + tid, Q - 1);        // tail lanes repeat the last query and write nothing
    qx[k] = q[3 * (size_t)i]; qy[k] = q[3 * (size_t)i + 1]; qz[k] = q[3 * (size_t)i + 2];
    best[k] = INFINITY;
    bidx[k] = t_begin;
  }
  for (int t0 = t_begin; t0 < t_end; t0 += kPointTile) {
    const int n = min(kPointTile, t_end - t0);
#ifndef GEOBI_DIST_UNIFORM_LOADS
    __syncthreads();
    for (int j = tid; j < n; j += kThreads) {
      const float* p = t + 3 * (size_t)(t0 + j);
      tile[j] = make_float4(p[0], p[1], p[2], 0.f);
    }
    __syncthreads();
#endif
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
#ifndef GEOBI_DIST_UNIFORM_LOADS
      const float4 tj = tile[j];
#else   // A/B variant (tools/build_variant.sh): no LDS tile, the wave-uniform target index makes these scalar loads
      const float* p = t + 3 * (size_t)(t0 + j);
      const float4 tj = make_float4(p[0], p[1], p[2], 0.f);
#endif
#pragma unroll
      for (int k = 0; k < kPointQpl; ++k) {
        const float d2 = pair_d2(qx[k], qy[k], qz[k], tj);
        const bool lt = d2 < best[k];
        best[k] = lt ? d2 : best[k];
        bidx[k] = lt ? t0 + j : bidx[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kPointQpl; ++k) {
    const int i = q0 + k * kThreads + tid;
    if (i < Q) {
      part_d2[(size_t)slice * Q + i] = best[k];
      part_idx[(size_t)slice * Q + i] = bidx[k];
    }
  }
}

// partials of the S slices in ascending order, strict <: the lowest index among equal distances survives
__global__ void nearest_reduce_kernel(const float* __restrict__ part_d2, const int* __restrict__ part_idx, int Q, int S,
                                      float* __restrict__ dist, int* __restrict__ idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Q) return;
  float best = part_d2[i];
  int b = part_idx[i];
  for (int s = 1; s < S; ++s) {
    const float d2 = part_d2[(size_t)s * Q + i];
    const int j = part_idx[(size_t)s * Q + i];
    if (d2 < best) { best = d2; b = j; }
  }
  dist[i] = sqrtf(best);
  if (idx) idx[i] = b;
}

// ---------------------------------------------------------------- point - point, confined to the parts of a union batch
// The search the correspondence-free losses need (code/network.py:369-370 chamfer_distance, :385-388 sided_distance) on
// a disjoint-union batch: queries of part p only meet targets of part p.  Same shape as nearest_point_kernel -- QPL
// queries per lane, the target tile in LDS read by broadcast, target slices, a strict-< reduction in ascending slice
// order -- and the same pair_d2, so for any part the answer is what nearest_point gives on that part's rows alone.  A
// workgroup belongs to ONE part (blocks are formed per part); the part table rides in the kernel arguments as the
// offsets of rotate_parts_kernel do (geom.hip): no copy of the host arrays, nothing out of stream order.
constexpr int kMaxSearchParts = 32;
struct PartsJob {
  int q_begin[kMaxSearchParts + 1];     // query rows of part k: q_begin[k] .. q_begin[k + 1]
  int t_begin[kMaxSearchParts + 1];     // target rows
  int block_begin[kMaxSearchParts + 1]; // first workgroup (blockIdx.x) of part k
  int tiles_per_slice[kMaxSearchParts];
  int slices[kMaxSearchParts];          // >= 1, no empty slice
  int n;
};

__global__ __launch_bounds__(kThreads) void nearest_parts_kernel(PartsJob job, const float* __restrict__ q,
                                                                 const float* __restrict__ t, int ld_part,
                                                                 float* __restrict__ part_d2, int* __restrict__ part_idx) {
  __shared__ float4 tile[kPointTile];
  const int tid = threadIdx.x;
  int p = 0;
  while (p + 1 < job.n && (int)blockIdx.x >= job.block_begin[p + 1]) ++p;      // wave-uniform
  const int slice = blockIdx.y;
  if (slice >= job.slices[p]) return;                                         // the whole workgroup leaves together
  const int q0 = job.q_begin[p] + ((int)blockIdx.x - job.block_begin[p]) * (kThreads * kPointQpl);
  const int q_end = job.q_begin[p + 1];
  const int span = job.tiles_per_slice[p] * kPointTile;
  const int t_begin = job.t_begin[p] + slice * span;
  const int t_end = min(job.t_begin[p + 1], t_begin + span);
  float qx[kPointQpl], qy[kPointQpl], qz[kPointQpl], best[kPointQpl];
  int bidx[kPointQpl];
#pragma unroll
  for (int k = 0; k < kPointQpl; ++k) {
    const int i = min(q0 + k * kThreads + tid, q_end - 1);    // tail lanes repeat the part's last query and write nothing
    qx[k] = q[3 * (size_t)i]; qy[k] = q[3 * (size_t)i + 1]; qz[k] = q[3 * (size_t)i + 2];
    best[k] = INFINITY;
    bidx[k] = t_begin;                                        // in range whatever the coordinates are (NaN included)
  }
  for (int t0 = t_begin; t0 < t_end; t0 += kPointTile) {
    const int n = min(kPointTile, t_end - t0);
    __syncthreads();
    for (int j = tid; j < n; j += kThreads) {
      const float* pt = t + 3 * (size_t)(t0 + j);
      tile[j] = make_float4(pt[0], pt[1], pt[2], 0.f);
    }
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < n; ++j) {
      const float4 tj = tile[j];
#pragma unroll
      for (int k = 0; k < kPointQpl; ++k) {
        const float d2 = pair_d2(qx[k], qy[k], qz[k], tj);
        const bool lt = d2 < best[k];
        best[k] = lt ? d2 : best[k];
        bidx[k] = lt ? t0 + j : bidx[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kPointQpl; ++k) {
    const int i = q0 + k * kThreads + tid;
    if (i < q_end) {
      part_d2[(size_t)slice * ld_part + i] = best[k];
      part_idx[(size_t)slice * ld_part + i] = bidx[k];
    }
  }
}

// the partials of a query's own part, slices in ascending order, strict <; the SQUARED distance goes out
__global__ __launch_bounds__(kThreads) void nearest_parts_reduce_kernel(PartsJob job, const float* __restrict__ part_d2,
                                                                        const int* __restrict__ part_idx, int ld_part,
                                                                        float* __restrict__ d2_out, int* __restrict__ idx) {
  __shared__ int s_begin[kMaxSearchParts + 1], s_slices[kMaxSearchParts];     // a lane indexes them by ITS part
  for (int k = threadIdx.x; k <= job.n; k += kThreads) s_begin[k] = job.q_begin[k];
  for (int k = threadIdx.x; k < job.n; k += kThreads) s_slices[k] = job.slices[k];
  __syncthreads();
  const int i = s_begin[0] + blockIdx.x * kThreads + threadIdx.x;
  if (i >= s_begin[job.n]) return;
  int lo = 0, hi = job.n - 1;
  while (lo < hi) {                                  // the part that holds row i (no part is empty)
    const int mid = (lo + hi + 1) >> 1;
    if (s_begin[mid] <= i) lo = mid; else hi = mid - 1;
  }
  const int S = s_slices[lo];
  float best = part_d2[i];
  int b = part_idx[i];
  for (int s = 1; s < S; ++s) {
    const float d2 = part_d2[(size_t)s * ld_part + i];
    const int j = part_idx[(size_t)s * ld_part + i];
    if (d2 < best) { best = d2; b = j; }
  }
  d2_out[i] = best;
  idx[i] = b;
}

// ---------------------------------------------------------------- point - triangle
// Record of one triangle (a, b, c), four float4:
//   r0 = (a, |ab|^2)   r1 = (ab, ab.ac)   r2 = (ac, |ac|^2)   r3 = (1/|ab|^2, 1/|ac|^2, 1/|bc|^2, 0)
// A triangle without area (|ab x ac|^2 <= 1e-10 |ab|^2 |ac|^2: its height is below 1e-5 of an edge) is stored as its
// longest edge (p, r) in the form a = p, b = c = r: every quantity the classification below derives for b and for c is
// then bit-identical, its three cross terms are exactly 0 and every query lands in corner a, corner b or edge ab --
// the point-segment distance, never a division by the vanished area.
__device__ __forceinline__ float dot_chain(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
  return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
}

__device__ __forceinline__ void triangle_record(const float* __restrict__ verts, const int* __restrict__ fv, int V, int f,
                                                float4* r0, float4* r1, float4* r2, float4* r3) {
#pragma clang fp contract(off)
  // the face table is range-checked by the caller; the clamp keeps a wrong one from reading outside `verts`
  const int ia = min(max(fv[3 * (size_t)f], 0), V - 1), ib = min(max(fv[3 * (size_t)f + 1], 0), V - 1),
            ic = min(max(fv[3 * (size_t)f + 2], 0), V - 1);
  float ax = verts[3 * (size_t)ia], ay = verts[3 * (size_t)ia + 1], az = verts[3 * (size_t)ia + 2];
  float bx = verts[3 * (size_t)ib], by = verts[3 * (size_t)ib + 1], bz = verts[3 * (size_t)ib + 2];
  float cx = verts[3 * (size_t)ic], cy = verts[3 * (size_t)ic + 1], cz = verts[3 * (size_t)ic + 2];
  float ux = bx - ax, uy = by - ay, uz = bz - az;           // ab
  float vx = cx - ax, vy = cy - ay, vz = cz - az;           // ac
  float wx = cx - bx, wy = cy - by, wz = cz - bz;           // bc
  // the same multiply-add chains as the dot products of tri_d2: a query AT corner b or c then finds d3 = d4 = 0 or
  // d5 = d6 = 0 exactly, lands in that corner's region and gets the distance 0.0
  float uu = dot_chain(ux, uy, uz, ux, uy, uz), vv = dot_chain(vx, vy, vz, vx, vy, vz),
        ww = dot_chain(wx, wy, wz, wx, wy, wz);
  const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
  if (nx * nx + ny * ny + nz * nz <= 1e-10f * uu * vv) {
    if (ww > uu && ww > vv) {          // bc is the longest edge: a <- b
      ax = bx; ay = by; az = bz;
      ux = wx; uy = wy; uz = wz; uu = ww;
    } else if (vv > uu) {              // ac
      ux = vx; uy = vy; uz = vz; uu = vv;
    }
    vx = ux; vy = uy; vz = uz; vv = uu;
    ww = 0.f;
  }
  const float uv = dot_chain(ux, uy, uz, vx, vy, vz);
  *r0 = make_float4(ax, ay, az, uu);
  *r1 = make_float4(ux, uy, uz, uv);
  *r2 = make_float4(vx, vy, vz, vv);
  *r3 = make_float4(uu > 0.f ? 1.0f / uu : 0.f, vv > 0.f ? 1.0f / vv : 0.f, ww > 0.f ? 1.0f / ww : 0.f, 0.f);
}

// Squared distance from p to the triangle: the region-classifying closest point of Ericson, Real-Time Collision
// Detection 5.1.5, in coordinates relative to corner a (translation-invariant: only p - a enters).  With
// d1 = ab.ap, d2 = ac.ap the other four dot products are d3 = ab.bp = d1 - |ab|^2, d4 = ac.bp = d2 - ab.ac,
// d5 = ab.cp = d1 - ab.ac, d6 = ac.cp = d2 - |ac|^2, and the three edge denominators d1 - d3, d2 - d6,
// (d4 - d3) + (d5 - d6) are the squared edge lengths, whose reciprocals come with the record.  The closest point is
// a + v ab + w ac; (v, w) is chosen by overriding the interior answer in reverse priority, branch-free.
__device__ __forceinline__ float tri_d2(float px, float py, float pz, float4 r0, float4 r1, float4 r2, float4 r3) {
#pragma clang fp contract(off)
  const float apx = px - r0.x, apy = py - r0.y, apz = pz - r0.z;
  const float d1 = dot_chain(r1.x, r1.y, r1.z, apx, apy, apz);
  const float d2 = dot_chain(r2.x, r2.y, r2.z, apx, apy, apz);
  const float d3 = d1 - r0.w, d4 = d2 - r1.w, d5 = d1 - r1.w, d6 = d2 - r2.w;
  const float vc = d1 * d4 - d3 * d2;
  const float vb = d5 * d2 - d1 * d6;
  const float va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  // interior
  const float inv = __builtin_amdgcn_rcpf(va + vb + vc);
  float v = vb * inv, w = vc * inv;
  // edge bc
  const bool on_bc = va <= 0.f && e43 >= 0.f && e56 >= 0.f;
  const float wbc = e43 * r3.z;
  v = on_bc ? 1.0f - wbc : v;
  w = on_bc ? wbc : w;
  // edge ac
  const bool on_ac = vb <= 0.f && d2 >= 0.f && d6 <= 0.f;
  v = on_ac ? 0.f : v;
  w = on_ac ? d2 * r3.y : w;
  // corner c
  const bool at_c = d6 >= 0.f && d5 <= d6;
  v = at_c ? 0.f : v;
  w = at_c ? 1.0f : w;
  // edge ab
  const bool on_ab = vc <= 0.f && d1 >= 0.f && d3 <= 0.f;
  v = on_ab ? d1 * r3.x : v;
  w = on_ab ? 0.f : w;
  // corner b
  const bool at_b = d3 >= 0.f && d4 <= d3;
  v = at_b ? 1.0f : v;
  w = at_b ? 0.f : w;
  // corner a
  const bool at_a = d1 <= 0.f && d2 <= 0.f;
  v = at_a ? 0.f : v;
  w = at_a ? 0.f : w;
  // a sliver whose cross terms are rounding noise must still answer with a point OF the triangle, and never NaN
  // (v_med3_f32 answers with the smaller finite operand when one operand is NaN)
  v = __builtin_amdgcn_fmed3f(v, 0.f, 1.0f);
  w = __builtin_amdgcn_fmed3f(w, 0.f, 1.0f - v);
  const float ex = __builtin_fmaf(-w, r2.x, __builtin_fmaf(-v, r1.x, apx));
  const float ey = __builtin_fmaf(-w, r2.y, __builtin_fmaf(-v, r1.y, apy));
  const float ez = __builtin_fmaf(-w, r2.z, __builtin_fmaf(-v, r1.z, apz));
  return __builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex));
}

__global__ __launch_bounds__(kThreads) void nearest_triangle_kernel(const float* __restrict__ q,
                                                                    const float* __restrict__ verts,
                                                                    const int* __restrict__ fv, int Q, int V, int F,
                                                                    int tiles_per_slice, float* __restrict__ part_d2,
                                                                    int* __restrict__ part_idx) {
  __shared__ float4 rec[4][kTriTile];
  const int tid = threadIdx.x;
  const int q0 = blockIdx.x * (kThreads * kTriQpl);
  const int slice = blockIdx.y;
  float qx[kTriQpl], qy[kTriQpl], qz[kTriQpl], best[kTriQpl];
  int bidx[kTriQpl];
  const int f_begin = slice * tiles_per_slice * kTriTile;
  const int f_end = min(F, f_begin + tiles_per_slice * kTriTile);
#pragma unroll
  for (int k = 0; k < kTriQpl; ++k) {
    const int i = min(q0 + k * kThreads + tid, Q - 1);
    qx[k] = q[3 * (size_t)i]; qy[k] = q[3 * (size_t)i + 1]; qz[k] = q[3 * (size_t)i + 2];
    best[k] = INFINITY;
    bidx[k] = f_begin;
  }
  static_assert(kTriTile == kThreads, "one thread stages one triangle of the tile");
  for (int f0 = f_begin; f0 < f_end; f0 += kTriTile) {
    const int n = min(kTriTile, f_end - f0);
    __syncthreads();
    if (tid < n) triangle_record(verts, fv, V, f0 + tid, &rec[0][tid], &rec[1][tid], &rec[2][tid], &rec[3][tid]);
    __syncthreads();
#pragma unroll 2
    for (int j = 0; j < n; ++j) {
      const float4 r0 = rec[0][j], r1 = rec[1][j], r2 = rec[2][j], r3 = rec[3][j];
#pragma unroll
      for (int k = 0; k < kTriQpl; ++k) {
        const float d2 = tri_d2(qx[k], qy[k], qz[k], r0, r1, r2, r3);
        const bool lt = d2 < best[k];
        best[k] = lt ? d2 : best[k];
        bidx[k] = lt ? f0 + j : bidx[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kTriQpl; ++k) {
    const int i = q0 + k * kThreads + tid;
    if (i < Q) {
      part_d2[(size_t)slice * Q + i] = best[k];
      part_idx[(size_t)slice * Q + i] = bidx[k];
    }
  }
}

// ---------------------------------------------------------------- sum / max of a distance vector
// fp64 accumulation, fixed order: thread-strided partial sums, an LDS tree per block, the blocks in ascending order.
__global__ __launch_bounds__(kThreads) void dist_summary_partial_kernel(const float* __restrict__ d, int64_t n,
                                                                        double* __restrict__ partial) {
  __shared__ double ssum[kThreads];
  __shared__ float smax[kThreads];
  double s = 0.0;
  float m = -INFINITY;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const float x = d[i];
    s += (double)x;
    m = fmaxf(m, x);
  }
  ssum[threadIdx.x] = s;
  smax[threadIdx.x] = m;
  __syncthreads();
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) {
      ssum[threadIdx.x] += ssum[threadIdx.x + h];
      smax[threadIdx.x] = fmaxf(smax[threadIdx.x], smax[threadIdx.x + h]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = ssum[0];
    partial[2 * blockIdx.x + 1] = (double)smax[0];
  }
}

__global__ void dist_summary_final_kernel(const double* __restrict__ partial, int blocks, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0, m = -INFINITY;
  for (int b = 0; b < blocks; ++b) {
    s += partial[2 * b];
    m = fmax(m, partial[2 * b + 1]);
  }
  out[0] = s;
  out[1] = m;
}

int summary_blocks(int64_t n) {
  const int64_t b = (n + 4 * kThreads - 1) / (4 * kThreads);
  return (int)(b < 1 ? 1 : (b > 512 ? 512 : b));
}

size_t partial_bytes(const Slicing& c, int64_t Q) {
  return align_up((size_t)c.slices * Q * sizeof(float)) + align_up((size_t)c.slices * Q * sizeof(int)) + 256;
}

}  // namespace

int nearest_slices(int64_t Q, int64_t T, int triangles) {
  if (Q <= 0 || T <= 0) return 0;
  return triangles ? choose_slices(Q, T, kTriQpl, kTriTile).slices : choose_slices(Q, T, kPointQpl, kPointTile).slices;
}

size_t nearest_ws_bytes(int64_t Q, int64_t T) {
  if (Q <= 0 || T <= 0) return 256;
  // enough for either kernel
  const Slicing a = choose_slices(Q, T, kPointQpl, kPointTile), b = choose_slices(Q, T, kTriQpl, kTriTile);
  return partial_bytes(a.slices > b.slices ? a : b, Q);
}

int nearest_point(const float* q, const float* t, int64_t Q, int64_t T, float* dist, int32_t* idx, void* ws,
                  size_t ws_bytes, hipStream_t s) {
  GEOBI_REQUIRE(Q > 0 && T > 0, "nearest_point: empty query or target set (Q = %lld, T = %lld)", (long long)Q, (long long)T);
  const Slicing c = choose_slices(Q, T, kPointQpl, kPointTile);
  Arena ar(ws, ws_bytes);
  float* pd = ar.take<float>((size_t)c.slices * Q);
  int* pi = ar.take<int>((size_t)c.slices * Q);
  GEOBI_REQUIRE(ar.ok() && pd && pi, "nearest_point: workspace too small (%zu bytes given, %zu needed)", ws_bytes, ar.off);
  nearest_point_kernel<<<dim3(c.qblocks, c.slices), kThreads, 0, s>>>(q, t, (int)Q, (int)T, c.tiles_per_slice, pd, pi);
  nearest_reduce_kernel<<<cdiv(Q, kThreads), kThreads, 0, s>>>(pd, pi, (int)Q, c.slices, dist, idx);
  GEOBI_LAUNCH_OK();
  return 0;
}

int parts_ptr_ok(const char* fn, const char* what, const int64_t* ptr, int P) {
  GEOBI_REQUIRE(P >= 1, "%s: P = %d parts (at least one)", fn, P);
  GEOBI_REQUIRE(ptr != nullptr && ptr[0] >= 0, "%s: %s is NULL or starts below 0", fn, what);
  for (int p = 0; p < P; ++p)
    GEOBI_REQUIRE(ptr[p + 1] > ptr[p], "%s: part %d of %s is empty (%lld .. %lld): an empty part is an error, not a launch", fn,
                  p, what, (long long)ptr[p], (long long)ptr[p + 1]);
  return 0;
}

namespace {
// slices every part would like: the workgroups of ALL parts together should fill the chip
int parts_want(const int64_t* qptr, int P) {
  int64_t qblocks = 0;
  for (int p = 0; p < P; ++p) qblocks += cdiv(qptr[p + 1] - qptr[p], (int64_t)kThreads * kPointQpl);
  int64_t want = (kTargetBlocks + qblocks - 1) / qblocks;
  return (int)(want > kMaxSlices ? kMaxSlices : (want < 1 ? 1 : want));
}
Slicing part_slices(int64_t Q, int64_t T, int want) {   // P = 1: exactly choose_slices
  Slicing c;
  c.qblocks = cdiv(Q, (int64_t)kThreads * kPointQpl);
  const int ntiles = cdiv(T, kPointTile);
  if (want > ntiles) want = ntiles;
  c.tiles_per_slice = cdiv(ntiles, want);
  c.slices = cdiv(ntiles, c.tiles_per_slice);
  return c;
}
bool parts_sane(const int64_t* qptr, const int64_t* tptr, int P) {
  if (P < 1 || !qptr || !tptr || qptr[0] < 0 || tptr[0] < 0) return false;
  for (int p = 0; p < P; ++p)
    if (qptr[p + 1] <= qptr[p] || tptr[p + 1] <= tptr[p]) return false;
  return qptr[P] <= INT32_MAX / 4 && tptr[P] <= INT32_MAX / 4;
}
}  // namespace

int nearest_parts_slices(const int64_t* qptr, const int64_t* tptr, int P) {
  if (!parts_sane(qptr, tptr, P)) return 0;
  const int want = parts_want(qptr, P);
  int smax = 0;
  for (int p = 0; p < P; ++p) {
    const int sl = part_slices(qptr[p + 1] - qptr[p], tptr[p + 1] - tptr[p], want).slices;
    smax = sl > smax ? sl : smax;
  }
  return smax;
}

size_t nearest_parts_ws_bytes(const int64_t* qptr, const int64_t* tptr, int P) {
  const int smax = nearest_parts_slices(qptr, tptr, P);
  if (smax == 0) return 256;
  return align_up((size_t)smax * qptr[P] * sizeof(float)) + align_up((size_t)smax * qptr[P] * sizeof(int)) + 256;
}

int nearest_parts(const float* q, const float* t, const int64_t* qptr, const int64_t* tptr, int P, float* d2, int32_t* idx,
                  void* ws, size_t ws_bytes, hipStream_t s) {
  GEOBI_TRY(parts_ptr_ok("nearest_parts", "qptr", qptr, P));
  GEOBI_TRY(parts_ptr_ok("nearest_parts", "tptr", tptr, P));
  const int want = parts_want(qptr, P);
  const int smax = nearest_parts_slices(qptr, tptr, P);
  const int ld = (int)qptr[P];
  Arena ar(ws, ws_bytes);
  float* pd = ar.take<float>((size_t)smax * ld);
  int* pi = ar.take<int>((size_t)smax * ld);
  GEOBI_REQUIRE(ar.ok() && pd && pi, "nearest_parts: workspace too small (%zu bytes given, %zu needed)", ws_bytes, ar.off);
  for (int base = 0; base < P; base += kMaxSearchParts) {
    PartsJob job;
    job.n = P - base < kMaxSearchParts ? P - base : kMaxSearchParts;
    int blocks = 0, sl_max = 0;
    for (int k = 0; k < job.n; ++k) {
      const int p = base + k;
      const Slicing c = part_slices(qptr[p + 1] - qptr[p], tptr[p + 1] - tptr[p], want);
      job.q_begin[k] = (int)qptr[p];
      job.t_begin[k] = (int)tptr[p];
      job.block_begin[k] = blocks;
      job.tiles_per_slice[k] = c.tiles_per_slice;
      job.slices[k] = c.slices;
      blocks += c.qblocks;
      sl_max = c.slices > sl_max ? c.slices : sl_max;
    }
    for (int k = job.n; k <= kMaxSearchParts; ++k) {      // the unused tail repeats the end: nothing is left unset
      job.q_begin[k] = (int)qptr[base + job.n];
      job.t_begin[k] = (int)tptr[base + job.n];
      job.block_begin[k] = blocks;
      if (k < kMaxSearchParts) { job.tiles_per_slice[k] = 1; job.slices[k] = 1; }
    }
    nearest_parts_kernel<<<dim3(blocks, sl_max), kThreads, 0, s>>>(job, q, t, ld, pd, pi);
    const int rows = job.q_begin[job.n] - job.q_begin[0];
    nearest_parts_reduce_kernel<<<cdiv(rows, kThreads), kThreads, 0, s>>>(job, pd, pi, ld, d2, idx);
  }
  GEOBI_LAUNCH_OK();
  return 0;
}

int nearest_triangle(const float* q, const float* verts, const int32_t* fv, int64_t Q, int64_t V, int64_t F, float* dist,
                     int32_t* face, void* ws, size_t ws_bytes, hipStream_t s) {
  GEOBI_REQUIRE(Q > 0 && V > 0 && F > 0, "nearest_triangle: empty query set or mesh (Q = %lld, V = %lld, F = %lld)",
                (long long)Q, (long long)V, (long long)F);
  const Slicing c = choose_slices(Q, F, kTriQpl, kTriTile);
  Arena ar(ws, ws_bytes);
  float* pd = ar.take<float>((size_t)c.slices * Q);
  int* pi = ar.take<int>((size_t)c.slices * Q);
  GEOBI_REQUIRE(ar.ok() && pd && pi, "nearest_triangle: workspace too small (%zu bytes given, %zu needed)", ws_bytes, ar.off);
  nearest_triangle_kernel<<<dim3(c.qblocks, c.slices), kThreads, 0, s>>>(q, verts, fv, (int)Q, (int)V, (int)F,
                                                                         c.tiles_per_slice, pd, pi);
  nearest_reduce_kernel<<<cdiv(Q, kThreads), kThreads, 0, s>>>(pd, pi, (int)Q, c.slices, dist, face);
  GEOBI_LAUNCH_OK();
  return 0;
}

size_t dist_summary_ws_bytes(int64_t n) { return align_up((size_t)summary_blocks(n) * 2 * sizeof(double)) + 256; }

int dist_summary(const float* dist, int64_t n, double* out, void* ws, size_t ws_bytes, hipStream_t s) {
  GEOBI_REQUIRE(n > 0, "dist_summary: empty vector");
  Arena ar(ws, ws_bytes);
  const int blocks = summary_blocks(n);
  double* partial = ar.take<double>((size_t)2 * blocks);
  GEOBI_REQUIRE(ar.ok() && partial, "dist_summary: workspace too small");
  dist_summary_partial_kernel<<<blocks, kThreads, 0, s>>>(dist, n, partial);
  dist_summary_final_kernel<<<1, 64, 0, s>>>(partial, blocks, out);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // namespace geobi
