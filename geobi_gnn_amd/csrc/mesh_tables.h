// The two sorted 48-bit tables that decim.hip and remesh.hip derive from the edge table of edge_table.h,
// into the buffers of its MeshTables:
//   pairs    the two directed pairs src << 24 | dst of every run head, sorted: the neighbours of a vertex in ascending id
//   corners  the keys v << 24 | f of every included face, sorted: the included faces at a vertex in ascending id
// mesh_rings.h walks them.
#pragma once
#include "edge_table.h"

namespace geobi {

// per sorted position: the two directed pairs of an edge head (kNoEdge elsewhere) and the count of the edges; with `locked`
// also the flags of the ends of an edge with n_e != 2 (every writer stores the same 1)
static __global__ void edge_heads_kernel(const uint64_t* __restrict__ keys, int n, uint64_t* __restrict__ pairs,
                                         int* __restrict__ locked, int* __restrict__ edge_count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool head = false;
  if (i < n) {
    const Run r = run_at(keys, n, i);
    head = r.head;
    uint64_t forth = kNoEdge, back = kNoEdge;
    if (head) {
      const int lo = edge_key_lo(keys[i]), hi = edge_key_hi(keys[i]);
      forth = keys[i];
      back = edge_key(hi, lo);
      if (locked != nullptr && (!r.two || r.three)) { locked[lo] = 1; locked[hi] = 1; }
    }
    pairs[2 * (size_t)i] = forth;
    pairs[2 * (size_t)i + 1] = back;
  }
  count_lanes(head, edge_count);
}

// the corner keys of every face (kNoEdge for a face that is not included); with `fkeep` its keep flag (= included), with
// `not_included` the count of the faces that are not
static __global__ void corner_keys_kernel(const int* __restrict__ fv, int F, int V, uint64_t* __restrict__ corners,
                                          int* __restrict__ fkeep, int* __restrict__ not_included) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  bool out = false;
  if (f < F) {
    int c[3];
    const bool inc = face_included(fv, nullptr, f, V, c[0], c[1], c[2]);
    for (int k = 0; k < 3; ++k) corners[3 * (size_t)f + k] = inc ? edge_key(c[k], f) : kNoEdge;
    if (fkeep != nullptr) fkeep[f] = inc ? 1 : 0;
    out = !inc;
  }
  if (not_included != nullptr) count_lanes(out, not_included);
}

// ---- the build steps (F > 0; they enqueue on s), after build_edge_table (edge_table.h)
// from the sorted edge table; *edge_count += the edges, locked (or NULL): see edge_heads_kernel
static inline int build_pair_table(const MeshTables& t, int64_t F, int* locked, int* edge_count, hipStream_t s) {
  const int n = (int)(3 * F);
  edge_heads_kernel<<<cdiv(n, kTableThreads), kTableThreads, 0, s>>>(t.k_out, n, t.p_in, locked, edge_count);
  GEOBI_LAUNCH_OK();
  return t.pair_sort.run(t.p_in, t.p_out, 2 * n, kEdgeKeyBits, s);
}
// fkeep, not_included (or NULL): see corner_keys_kernel
static inline int build_corner_table(const MeshTables& t, const int32_t* faces, int64_t F, int64_t V, int* fkeep,
                                     int* not_included, hipStream_t s) {
  corner_keys_kernel<<<cdiv(F, kTableThreads), kTableThreads, 0, s>>>(faces, (int)F, (int)V, t.c_in, fkeep, not_included);
  GEOBI_LAUNCH_OK();
  return t.corner_sort.run(t.c_in, t.c_out, 3 * F, kEdgeKeyBits, s);
}

}  // namespace geobi
