// The undirected edge table of the mesh tools, shared by topo.hip, clean.hip, subdiv.hip, decim.hip,
// remesh.hip and fill.hip: which faces are included, which key a slot gets, how a run of the sorted table is read, how an index comes out
// of a key -- and MeshTables, the buffers of the table (and of the two tables mesh_tables.h derives from it) with their carve
// and its sorts.  Sorting the slots stably on kEdgeKeyBits bits makes a run of equal keys one edge, its length the number
// of claimants, the claimants in ascending slot order and the run heads ascend with (lo, hi).
#pragma once
#include "device_steps.h"

namespace geobi {

// the corners of face f; true when they lie in [0, V), differ, and the face's state (if any) is "kept"
__device__ __forceinline__ bool face_included(const int* __restrict__ fv, const int* __restrict__ state, int f, int V,
                                              int& a, int& b, int& c) {
  a = fv[3 * (size_t)f]; b = fv[3 * (size_t)f + 1]; c = fv[3 * (size_t)f + 2];
  const bool in_range = (unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned)c < (unsigned)V;
  return in_range && a != b && b != c && c != a && (state == nullptr || state[f] == kKept);
}

// the three edge slots of every face: slot 3f + k joins corner k and corner k + 1 mod 3, key lo << 24 | hi (kNoEdge for
// a face that is not included), value slot << 1 | direction bit (0 when the face walks lo -> hi)
static __global__ void edge_slots_kernel(const int* __restrict__ fv, const int* __restrict__ state, int F, int V,
                                         uint64_t* __restrict__ keys, int* __restrict__ vals) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  int c[3];
  const bool inc = face_included(fv, state, f, V, c[0], c[1], c[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int a = c[k], b = c[(k + 1) % 3];
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    keys[3 * (size_t)f + k] = inc ? edge_key(lo, hi) : kNoEdge;
    vals[3 * f + k] = (3 * f + k) << 1 | (a < b ? 0 : 1);
  }
}

// The two ends of a key, for use as indices.  Each passes through a register the optimiser cannot see into.  With the
// 24-bit mask in view, hipcc 7.2 for gfx950 lowered `points[3 * (size_t)hi]` to ONE v_mad_u64_u32 on the unmasked low word
// of the key (the multiply-by-24-bit-value combine drops the mask, then a full 32 x 32 -> 64 multiply-add is selected):
// the address then carries the low 8 bits of `lo` as bits 24 .. 31 of the index, far outside the array.
__device__ __forceinline__ int index_from_key(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ int edge_key_lo(uint64_t key) { return index_from_key((int)(key >> 24 & 0xffffffull)); }
__device__ __forceinline__ int edge_key_hi(uint64_t key) { return index_from_key((int)(key & 0xffffffull)); }

// what sorted position i is in its run: the head of an edge, followed by a second and a third claimant
struct Run { bool head, two, three; };
__device__ __forceinline__ Run run_at(const uint64_t* __restrict__ keys, int n, int i) {
  const uint64_t key = keys[i];
  Run r;
  r.head = key != kNoEdge && (i == 0 || keys[i - 1] != key);
  r.two = i + 1 < n && keys[i + 1] == key;
  r.three = r.two && i + 2 < n && keys[i + 2] == key;
  return r;
}

// ---- the buffers of the three sorted 48-bit tables: the edges always, the directed pairs and the corner keys
// (mesh_tables.h) where the unit asks for them.  A unit embeds MeshTables in its own buffers.
constexpr int kTableThreads = 256;
struct MeshTables {
  uint64_t *k_in, *k_out;          // [3F] edge keys before and after the sort
  int *v_in, *v_out;               // [3F] their values
  uint64_t *p_in, *p_out;          // [6F] directed pairs, NULL when not asked for
  uint64_t *c_in, *c_out;          // [3F] corner keys, NULL when not asked for
  PairSort<uint64_t, int> edge_sort; KeySort<uint64_t> pair_sort, corner_sort;
};
// the carve of the tables a unit asks for: the takes run in the order written, as in a unit's own braced list
template <bool kPairs, bool kCorners>
static inline MeshTables carve_tables(Arena& a, int64_t F) {
  const int64_t n = 3 * F;
  MeshTables t = {a.take<uint64_t>(n), a.take<uint64_t>(n), a.take<int>(n), a.take<int>(n)};
  t.edge_sort = PairSort<uint64_t, int>::take(a, n, kEdgeKeyBits);
  if constexpr (kPairs) {
    t.p_in = a.take<uint64_t>(2 * n); t.p_out = a.take<uint64_t>(2 * n);
    t.pair_sort = KeySort<uint64_t>::take(a, 2 * n, kEdgeKeyBits);
  }
  if constexpr (kCorners) {
    t.c_in = a.take<uint64_t>(n); t.c_out = a.take<uint64_t>(n);
    t.corner_sort = KeySort<uint64_t>::take(a, n, kEdgeKeyBits);
  }
  return t;
}

// the build steps of the edge table (F > 0; they enqueue on s).  k_in / v_in -> k_out / v_out: the one sort
static inline int sort_edge_table(const MeshTables& t, int64_t F, hipStream_t s) {
  return t.edge_sort.run(t.k_in, t.k_out, t.v_in, t.v_out, 3 * F, kEdgeKeyBits, s);
}
static inline int build_edge_table(const MeshTables& t, const int32_t* faces, const int32_t* state, int64_t F, int64_t V,
                                   hipStream_t s) {
  edge_slots_kernel<<<cdiv(F, kTableThreads), kTableThreads, 0, s>>>(faces, state, (int)F, (int)V, t.k_in, t.v_in);
  GEOBI_LAUNCH_OK();
  return sort_edge_table(t, F, s);
}

}  // namespace geobi
