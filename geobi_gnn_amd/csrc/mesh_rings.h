// What subdiv.hip, decim.hip (4o) and remesh.hip (4p) share on the device: fp64 points, squared edge
// lengths and face normals in the one stated order, the float32 midpoint, and the walks over the sorted corner and pair
// tables of mesh_tables.h (the included faces at a vertex, the neighbours of a vertex, both in ascending id).  Every index
// taken out of a key passes through index_from_key (edge_table.h).  The ranked selection over these walks is mesh_select.h.
#pragma once
#include "common.h"
#include "edge_table.h"

#pragma clang fp contract(off)

namespace geobi {

struct P3 { double x, y, z; };

__device__ __forceinline__ P3 point_of(const float* __restrict__ points, int v) {
  return {(double)points[3 * (size_t)v], (double)points[3 * (size_t)v + 1], (double)points[3 * (size_t)v + 2]};
}

// fp64 squared length of the edge lo - hi from its float32 ends: hi - lo per axis, (dx dx + dy dy) + dz dz
__device__ __forceinline__ double edge_len2(const float* __restrict__ points, int lo, int hi) {
#pragma clang fp contract(off)
  const P3 a = point_of(points, lo), b = point_of(points, hi);
  const double dx = b.x - a.x, dy = b.y - a.y, dz = b.z - a.z;
  return (dx * dx + dy * dy) + dz * dz;
}

// n = (b - a) x (c - a), every component two products and one subtraction; -> s = (nx nx + ny ny) + nz nz
__device__ __forceinline__ double normal_of(const P3& a, const P3& b, const P3& c, P3& n) {
#pragma clang fp contract(off)
  const double ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
  const double wx = c.x - a.x, wy = c.y - a.y, wz = c.z - a.z;
  n.x = uy * wz - uz * wy;
  n.y = uz * wx - ux * wz;
  n.z = ux * wy - uy * wx;
  return (n.x * n.x + n.y * n.y) + n.z * n.z;
}

__device__ __forceinline__ double dot_of(const P3& a, const P3& b) {
#pragma clang fp contract(off)
  return (a.x * b.x + a.y * b.y) + a.z * b.z;
}

__device__ __forceinline__ float midpoint(float a, float b) {
#pragma clang fp contract(off)
  return 0.5f * a + 0.5f * b;
}

// the first position of a sorted list that is not below x
__device__ __forceinline__ int lower_bound(const uint64_t* __restrict__ a, int n, uint64_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// a corner key v << 24 | f or a directed pair src << 24 | dst: the owner (2^24 - 1 for kNoEdge: never a vertex) and the
// other field as an index (edge_table.h: index_from_key)
__device__ __forceinline__ int owner_of(uint64_t key) { return (int)(key >> 24); }
__device__ __forceinline__ int item_of(uint64_t key) { return index_from_key((int)(key & 0xffffffull)); }

// the faces at v other than those that hold `other` (none for other < 0) keep the side of their normal when v moves to `at`
__device__ __forceinline__ bool no_flip(const float* __restrict__ points, const int* __restrict__ fv,
                                        const uint64_t* __restrict__ corners, int n, int v, int other, const P3& at) {
#pragma clang fp contract(off)
  bool ok = true;
  for (int j = lower_bound(corners, n, (uint64_t)v << 24); j < n && owner_of(corners[j]) == v; ++j) {
    const int f = item_of(corners[j]);
    const int c0 = fv[3 * (size_t)f], c1 = fv[3 * (size_t)f + 1], c2 = fv[3 * (size_t)f + 2];
    if (c0 == other || c1 == other || c2 == other) continue;
    const P3 a = point_of(points, c0), b = point_of(points, c1), c = point_of(points, c2);
    P3 was, now;
    if (normal_of(a, b, c, was) == 0.0) continue;
    normal_of(c0 == v ? at : a, c1 == v ? at : b, c2 == v ? at : c, now);
    if (!((was.x * now.x + was.y * now.y) + was.z * now.z > 0.0)) ok = false;
  }
  return ok;
}

// the LINK and VALENCE tests of 4o in one merge walk over the two neighbour lists: lo and hi share exactly two
// neighbours, both of valence >= 4
__device__ __forceinline__ bool link_and_valence(const uint64_t* __restrict__ pairs, int n_pairs, int lo, int hi) {
  bool valid = true;
  int a = lower_bound(pairs, n_pairs, (uint64_t)lo << 24), b = lower_bound(pairs, n_pairs, (uint64_t)hi << 24);
  int shared = 0;
  while (a < n_pairs && b < n_pairs && owner_of(pairs[a]) == lo && owner_of(pairs[b]) == hi) {
    const int da = item_of(pairs[a]), db = item_of(pairs[b]);
    if (da == db) {
      ++shared;
      const int w = lower_bound(pairs, n_pairs, (uint64_t)da << 24);
      if (!(w + 3 < n_pairs && owner_of(pairs[w + 3]) == da)) valid = false;     // valence below 4
      ++a; ++b;
    } else if (da < db) {
      ++a;
    } else {
      ++b;
    }
  }
  return valid && shared == 2;
}

}  // namespace geobi
