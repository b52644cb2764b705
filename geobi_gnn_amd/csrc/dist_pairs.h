// The pair functions of the nearest searches: the squared distance of a query to ONE target point (pair_d2) or ONE
// triangle record (triangle_record, tri_d2).  Shared TEXT: dist.hip (the all-pairs walk) and grid.hip (the grid in front
// of it) include this header, so a pair's d2 is formed by the same instruction sequence in both and the
// grid's answer is the all-pairs answer bit for bit.  Contraction is off in every function and every fused multiply-add
// is written out.
#pragma once
#include "common.h"

#include <math.h>

namespace geobi {

// ---------------------------------------------------------------- point - point
__device__ __forceinline__ float pair_d2(float qx, float qy, float qz, float4 t) {
#pragma clang fp contract(off)
  const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
  return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
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

}  // namespace geobi
