// Points on the faces of a mesh from (face, barycentric) pairs, and the gradient back to the vertices that carry them: the
// differentiable step of the sampled Chamfer loss.  The sampler (sample.hip) draws (face, bary) on the
// detached prediction; they are constants of the gradient, as the arg-min maps of the Chamfer distance are.
//
//   forward    x_i = fma(b_i2, c, fma(b_i1, b, b_i0 * a))   (a, b, c) = points[fv[face_i]]: the sampler's own formula, so
//              on the sampler's (face, bary) the sampler's points come back bit for bit.  A row whose face is outside
//              [0, F) (the sampler's -1 for a mesh without area) is zeros.
//   keys       key[3 i + k] = fv[face_i][k] clamped into [0, V); V ("no vertex") for a row whose face is outside [0, F).
//              geobi_segment_csr over them with nseg = V gives the inverse lists vertex -> entries e = 3 i + k, ascending;
//              the key V sorts behind every list.
//   backward   gp_v = sum over the entries e = 3 i + k of v's list, ascending, of bary[e] * gx_i: the products (exact:
//              two floats in fp64) and the sum in fp64, rounded once.  One lane per vertex writes its row exactly once,
//              zeros for a vertex no sample touches: no atomics, the same bits for every run and grid shape.  The mean
//              list is 3 n / V entries long; a hub vertex is only slower.
//
// What the kernels read through an index is clamped to the arrays: a foreign table gives wrong numbers, never a read outside.
#include "common.h"
#include "../../include/geobi_hip.h"

namespace geobi {

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__global__ __launch_bounds__(kThreads) void bary_points_kernel(const float* __restrict__ points, const int* __restrict__ fv,
                                                               const int* __restrict__ face, const float* __restrict__ bary,
                                                               int V, int F, int n, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const size_t o = 3 * (size_t)i;
  const int f = face[i];
  if (f < 0 || f >= F) {
    out[o] = out[o + 1] = out[o + 2] = 0.f;
    return;
  }
  const size_t ia = 3 * (size_t)clampi(fv[3 * (size_t)f], V), ib = 3 * (size_t)clampi(fv[3 * (size_t)f + 1], V),
               ic = 3 * (size_t)clampi(fv[3 * (size_t)f + 2], V);
  const float b0 = bary[o], b1 = bary[o + 1], b2 = bary[o + 2];
  for (int k = 0; k < 3; ++k) out[o + k] = fmaf(b2, points[ic + k], fmaf(b1, points[ib + k], b0 * points[ia + k]));
}

__global__ __launch_bounds__(kThreads) void bary_keys_kernel(const int* __restrict__ fv, const int* __restrict__ face, int V,
                                                             int F, int n, int* __restrict__ keys) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int f = face[i];
  const bool on = f >= 0 && f < F;
  for (int k = 0; k < 3; ++k) keys[3 * (size_t)i + k] = on ? clampi(fv[3 * (size_t)f + k], V) : V;
}

__global__ __launch_bounds__(kThreads) void bary_points_bwd_kernel(const float* __restrict__ bary, const float* __restrict__ gx,
                                                                   const int* __restrict__ segptr,
                                                                   const int* __restrict__ members, int V, int n_entries,
                                                                   float* __restrict__ gp) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= V) return;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  const int k_end = min(segptr[v + 1], n_entries);
  for (int k = max(segptr[v], 0); k < k_end; ++k) {
    const int e = clampi(members[k], n_entries);         // entry 3 i + k of bary, row i = e / 3 of gx
    const size_t r = 3 * (size_t)(e / 3);
    const double b = (double)bary[e];
    sx += b * (double)gx[r]; sy += b * (double)gx[r + 1]; sz += b * (double)gx[r + 2];
  }
  gp[3 * (size_t)v] = (float)sx;
  gp[3 * (size_t)v + 1] = (float)sy;
  gp[3 * (size_t)v + 2] = (float)sz;
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

int geobi_bary_points(const float* points, const int32_t* fv, const int32_t* face, const float* bary, int64_t V, int64_t F,
                      int64_t n, float* out, void* stream) {
  GEOBI_SIZES(F > V ? F : V, 0);
  GEOBI_SIZES(n, 0);
  GEOBI_REQUIRE(F >= 1 && V >= 1, "%s: F = %lld faces, V = %lld vertices (at least one of each)", __func__, (long long)F,
                (long long)V);
  if (n == 0) return 0;
  GEOBI_NOTNULL(points); GEOBI_NOTNULL(fv); GEOBI_NOTNULL(face); GEOBI_NOTNULL(bary); GEOBI_NOTNULL(out);
  bary_points_kernel<<<cdiv(n, kThreads), kThreads, 0, as_stream(stream)>>>(points, fv, face, bary, (int)V, (int)F, (int)n, out);
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_bary_keys(const int32_t* fv, const int32_t* face, int64_t V, int64_t F, int64_t n, int32_t* keys, void* stream) {
  GEOBI_SIZES(F > V ? F : V, 0);
  GEOBI_SIZES(n, 0);
  GEOBI_REQUIRE(F >= 1 && V >= 1, "%s: F = %lld faces, V = %lld vertices (at least one of each)", __func__, (long long)F,
                (long long)V);
  if (n == 0) return 0;
  GEOBI_NOTNULL(fv); GEOBI_NOTNULL(face); GEOBI_NOTNULL(keys);
  bary_keys_kernel<<<cdiv(n, kThreads), kThreads, 0, as_stream(stream)>>>(fv, face, (int)V, (int)F, (int)n, keys);
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_bary_points_bwd(const float* bary, const float* gx, const int32_t* segptr, const int32_t* members, int64_t V,
                          int64_t n, float* gp, void* stream) {
  GEOBI_SIZES(V, 0);
  GEOBI_SIZES(n, 0);
  GEOBI_REQUIRE(V >= 1, "%s: V = %lld vertices (at least one)", __func__, (long long)V);
  GEOBI_NOTNULL(segptr); GEOBI_NOTNULL(gp);
  if (n > 0) { GEOBI_NOTNULL(bary); GEOBI_NOTNULL(gx); GEOBI_NOTNULL(members); }
  // n == 0: every list is empty (segptr is all zeros) and every row of gp is written as zeros
  bary_points_bwd_kernel<<<cdiv(V, kThreads), kThreads, 0, as_stream(stream)>>>(bary, gx, segptr, members, (int)V, (int)(3 * n),
                                                                                gp);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
