// Ranked independent selection, shared by decim.hip (where it is described) and remesh.hip (4p).  The
// candidates are sorted positions of the edge table, ranked by the unit's own sort; a sweep selects every live candidate
// whose rank is the least over the closed rings of its footprint and retires the candidates those rings touch:
//   m1      atomicMin of the ranks into m1 at the footprint vertices (nobody reads m1 in that launch)
//   m2      per vertex the least m1 over its closed ring
//   select  a live candidate with the least m2 of its footprint == its rank is selected and blocks those rings
//   die     a live candidate with a blocked footprint vertex is no longer live
// A candidate descriptor is a plain struct of pointers with
//   kSize                  the footprint size
//   footprint(i, v)        the kSize vertices of the candidate at position i, each below V and each taken out of its key
//                          through edge_key_lo / edge_key_hi / index_from_key (edge_table.h)
//   record(i)              what a selected candidate notes besides its state (it is the head of a run of two: i + 1 < n)
#pragma once
#include "mesh_rings.h"

namespace geobi {

constexpr int kSelectThreads = 256;
constexpr int kNone = 0x7f7f7f7f;                   // no rank: what a memset of 0x7f leaves, above every position
constexpr uint64_t kNoCandidate = ~0ull;            // the sort key of what is no valid candidate: sorts last
enum State { kLive = 1, kSelected = 2 };
// a unit's device counters: [0, kSweepBase) its own, [kSweepBase + s] the candidates selected in sweep s
constexpr int kSweepBase = 8, kDevCounts = 16;

// order[j] = the position of the candidate of rank j: rank and state per position
static __global__ void rank_kernel(const uint64_t* __restrict__ sorted_key, const int* __restrict__ order, int n,
                                   int* __restrict__ rank, int* __restrict__ state) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int i = order[j];
  if ((unsigned)i >= (unsigned)n) return;
  const bool valid = sorted_key[j] != kNoCandidate;
  rank[i] = valid ? j : kNone;
  state[i] = valid ? kLive : 0;
}

__device__ __forceinline__ void block_ring(const uint64_t* __restrict__ pairs, int n_pairs, int v, int* __restrict__ blocked) {
  blocked[v] = 1;
  for (int j = lower_bound(pairs, n_pairs, (uint64_t)v << 24); j < n_pairs && owner_of(pairs[j]) == v; ++j)
    blocked[item_of(pairs[j])] = 1;
}

template <typename Candidate>
__global__ void select_m1_kernel(const Candidate c, int n, const int* __restrict__ state, const int* __restrict__ rank,
                                 int* __restrict__ m1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (state[i] & kLive) == 0) return;
  int v[Candidate::kSize];
  c.footprint(i, v);
#pragma unroll
  for (int k = 0; k < Candidate::kSize; ++k) atomicMin(m1 + v[k], rank[i]);
}

// m2[v] = the least m1 over the closed ring of v
static __global__ void ring_min_kernel(const int* __restrict__ m1, int V, const uint64_t* __restrict__ pairs, int n_pairs,
                                       int* __restrict__ m2) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  int m = m1[v];
  for (int j = lower_bound(pairs, n_pairs, (uint64_t)v << 24); j < n_pairs && owner_of(pairs[j]) == v; ++j) {
    const int w = m1[item_of(pairs[j])];
    m = w < m ? w : m;
  }
  m2[v] = m;
}

template <typename Candidate>
__global__ void select_kernel(const Candidate c, int n, const int* __restrict__ rank, const int* __restrict__ m2,
                              const uint64_t* __restrict__ pairs, int n_pairs, int* __restrict__ state,
                              int* __restrict__ blocked, int* __restrict__ selected_count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool selected = false;
  if (i + 1 < n && (state[i] & kLive) != 0) {       // a live candidate is the head of a run of two
    int v[Candidate::kSize];
    c.footprint(i, v);
    int least = m2[v[0]];
#pragma unroll
    for (int k = 1; k < Candidate::kSize; ++k) least = m2[v[k]] < least ? m2[v[k]] : least;
    selected = least == rank[i];
    if (selected) {
      state[i] |= kSelected;
#pragma unroll
      for (int k = 0; k < Candidate::kSize; ++k) block_ring(pairs, n_pairs, v[k], blocked);
      c.record(i);
    }
  }
  count_lanes(selected, selected_count);
}

template <typename Candidate>
__global__ void select_die_kernel(const Candidate c, int n, const int* __restrict__ blocked, int* __restrict__ state) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (state[i] & kLive) == 0) return;
  int v[Candidate::kSize];
  c.footprint(i, v);
  bool hit = false;
#pragma unroll
  for (int k = 0; k < Candidate::kSize; ++k) hit = hit || blocked[v[k]] != 0;
  if (hit) state[i] &= ~kLive;
}

// `sweeps` sweeps over the n positions and V vertices; rank and state come from rank_kernel, blocked starts as zeros,
// sweep_counts[s] += the candidates selected in sweep s
template <typename Candidate>
static inline int run_select_sweeps(const Candidate& c, int sweeps, int n, int64_t V, const uint64_t* pairs, int n_pairs,
                                    const int* rank, int* state, int* m1, int* m2, int* blocked, int* sweep_counts,
                                    hipStream_t s) {
  constexpr int kT = kSelectThreads;
  for (int sweep = 0; sweep < sweeps && V > 0; ++sweep) {
    GEOBI_HIP(hipMemsetAsync(m1, 0x7f, sizeof(int) * (size_t)V, s));             // kNone
    select_m1_kernel<<<cdiv(n, kT), kT, 0, s>>>(c, n, state, rank, m1);
    GEOBI_LAUNCH_OK();
    ring_min_kernel<<<cdiv(V, kT), kT, 0, s>>>(m1, (int)V, pairs, n_pairs, m2);
    GEOBI_LAUNCH_OK();
    select_kernel<<<cdiv(n, kT), kT, 0, s>>>(c, n, rank, m2, pairs, n_pairs, state, blocked, sweep_counts + sweep);
    GEOBI_LAUNCH_OK();
    select_die_kernel<<<cdiv(n, kT), kT, 0, s>>>(c, n, blocked, state);
    GEOBI_LAUNCH_OK();
  }
  return 0;
}

}  // namespace geobi
