// Closest points on given faces: for every query the point of ONE triangle nearest to it, as
// barycentric weights, as a position and as a distance.  The triangle is what geobi_nearest_triangle (dist.hip) returned;
// that all-pairs search stays the hot path and keeps its bits, this is the O(Q) step behind it.  The rules are stated in
// include/geobi_hip.h (geobi_closest_on_faces); tests/project_model.py restates them in plain Python and every output is
// compared bit for bit.
//
// One lane per query.  Every float step is fp64 from the float32 inputs in one stated order (contraction off, __ddiv_rn /
// __dsqrt_rn); the position alone is float32: the fma chain of geobi_bary_points (surfpoints.hip) on the float32 weights,
// so that geobi_bary_points on (face, bary) gives the same bits here and the counterpart on any paired vertex array.
// Nothing depends on launch geometry.  Every index is bounded: i < Q, the face is tested against [0, F) before its row is
// read, the ids of the row are clamped into [0, V).
#include "common.h"
#include "../../include/geobi_hip.h"

#pragma clang fp contract(off)

namespace geobi {

namespace {

constexpr int kThreads = 256;

struct D3 { double x, y, z; };

__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__device__ __forceinline__ D3 sub(const D3& u, const D3& w) {
#pragma clang fp contract(off)
  return {u.x - w.x, u.y - w.y, u.z - w.z};
}

__device__ __forceinline__ double dot(const D3& u, const D3& w) {
#pragma clang fp contract(off)
  return (u.x * w.x + u.y * w.y) + u.z * w.z;
}

// num / den, correctly rounded; 0 for a zero denominator or a NaN
__device__ __forceinline__ double weight(double num, double den) {
  if (den == 0.0) return 0.0;
  const double t = __ddiv_rn(num, den);
  return t == t ? t : 0.0;
}

__global__ __launch_bounds__(kThreads) void closest_on_faces_kernel(const float* __restrict__ q, const float* __restrict__ verts,
                                                                    const int* __restrict__ fv, const int* __restrict__ face,
                                                                    int Q, int V, int F, float* __restrict__ bary,
                                                                    float* __restrict__ point, float* __restrict__ dist) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= Q) return;
  const size_t o = 3 * (size_t)i;
  const int f = face[i];
  if (f < 0 || f >= F) {
    for (int k = 0; k < 3; ++k) bary[o + k] = point[o + k] = 0.f;
    dist[i] = 0.f;
    return;
  }
  const size_t ia = 3 * (size_t)clampi(fv[3 * (size_t)f], V), ib = 3 * (size_t)clampi(fv[3 * (size_t)f + 1], V),
               ic = 3 * (size_t)clampi(fv[3 * (size_t)f + 2], V);
  const float qx = q[o], qy = q[o + 1], qz = q[o + 2];
  double v = 0.0, w = 0.0;
  float d = INFINITY;
  if (isfinite(qx) && isfinite(qy) && isfinite(qz)) {
    const D3 p = {(double)qx, (double)qy, (double)qz};
    const D3 a = {(double)verts[ia], (double)verts[ia + 1], (double)verts[ia + 2]};
    const D3 b = {(double)verts[ib], (double)verts[ib + 1], (double)verts[ib + 2]};
    const D3 c = {(double)verts[ic], (double)verts[ic + 1], (double)verts[ic + 2]};
    const D3 ab = sub(b, a), ac = sub(c, a), ap = sub(p, a), bp = sub(p, b), cp = sub(p, c);
    const double d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
    const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0 && d2 <= 0.0) {                                        // corner a
    } else if (d3 >= 0.0 && d4 <= d3) {                                  // corner b
      v = 1.0;
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {                    // edge ab
      v = weight(d1, d1 - d3);
    } else if (d6 >= 0.0 && d5 <= d6) {                                  // corner c
      w = 1.0;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {                    // edge ac
      w = weight(d2, d2 - d6);
    } else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {          // edge bc
      w = weight(d4 - d3, (d4 - d3) + (d5 - d6));
      v = 1.0 - w;
    } else {                                                             // inside
      const double den = (va + vb) + vc;
      v = weight(vb, den);
      w = weight(vc, den);
    }
    v = fmin(fmax(v, 0.0), 1.0);
    w = fmin(fmax(w, 0.0), 1.0 - v);
    const double ex = p.x - ((a.x + v * ab.x) + w * ac.x), ey = p.y - ((a.y + v * ab.y) + w * ac.y),
                 ez = p.z - ((a.z + v * ab.z) + w * ac.z);
    d = (float)__dsqrt_rn((ex * ex + ey * ey) + ez * ez);
  }
  const float b0 = (float)((1.0 - v) - w), b1 = (float)v, b2 = (float)w;
  bary[o] = b0; bary[o + 1] = b1; bary[o + 2] = b2;
  for (int k = 0; k < 3; ++k) point[o + k] = fmaf(b2, verts[ic + k], fmaf(b1, verts[ib + k], b0 * verts[ia + k]));
  dist[i] = d;
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

int geobi_closest_on_faces(const float* q, const float* verts, const int32_t* fv, const int32_t* face, int64_t Q, int64_t V,
                           int64_t F, float* bary, float* point, float* dist, void* stream) {
  GEOBI_SIZES(F > V ? F : V, 0);
  GEOBI_SIZES(Q, 0);
  GEOBI_REQUIRE(Q >= 1 && F >= 1 && V >= 1, "%s: Q = %lld queries, F = %lld faces, V = %lld vertices (at least one of each)",
                __func__, (long long)Q, (long long)F, (long long)V);
  GEOBI_NOTNULL(q); GEOBI_NOTNULL(verts); GEOBI_NOTNULL(fv); GEOBI_NOTNULL(face);
  GEOBI_NOTNULL(bary); GEOBI_NOTNULL(point); GEOBI_NOTNULL(dist);
  closest_on_faces_kernel<<<cdiv(Q, kThreads), kThreads, 0, as_stream(stream)>>>(q, verts, fv, face, (int)Q, (int)V, (int)F, bary,
                                                                                 point, dist);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
