// The slots of the undirected edge table, shared by topo.hip and subdiv.hip (4n): which faces are
// included, which key a slot gets.  Sorting the slots stably on kEdgeKeyBits bits makes a run of equal keys one edge, its
// length the number of claimants, the claimants in ascending slot order and the run heads ascend with (lo, hi).
#pragma once
#include "common.h"

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

}  // namespace geobi
