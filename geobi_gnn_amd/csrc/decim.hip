// Triangle-mesh simplification on the device: rounds of independent quadric edge collapses, one
// round per plan + emit.  The rules are stated in include/geobi_hip.h (geobi_decim_*); tests/decim_model.py restates them
// sequentially and every output is compared bit for bit.
//
// The topology is integer-exact and independent of launch geometry; every float step is fp64 in one stated order
// (contraction off throughout, __dsqrt_rn / __ddiv_rn, no float atomics):
//   tables   the edge table of edge_table.h: a run is an edge, and an edge is known by the sorted position of its head,
//            which orders the edges as their ids do; the corner keys and the directed pairs of mesh_tables.h (the included
//            faces and the neighbours of a vertex in ascending id, both one binary search away).  The corner kernel also
//            writes the keep flags, the heads kernel the lock flags
//   values   one lane per vertex sums its quadric over its corner run; one lane per edge head picks the placement and
//            runs the link, valence and flip tests; two stable sorts (hash, then cost) rank the valid candidates
//   select   GEOBI_DECIM_SWEEPS sweeps of mesh_select.h over the two ends of an edge: atomicMin of the ranks into m1
//            (nobody reads m1 in that launch), m2 per vertex, select + block (writes `blocked`, reads m2), die (reads
//            `blocked`)
//   budget   the selected flags in rank order, scanned; roles of the vertices, keep flags of vertices and faces, scanned
//   emit     one lane per vertex, per face and per output row
// Every index is bounded: corners are below V (face_included), slots below 3F, vertices and faces taken out of a key were
// put into it from such a corner or face, output rows are checked against the sizes the caller read from the counts.
//
// geobi_decim_plan_short is the same round with another candidate kernel: the cost is the squared length
// of an edge below `low`, the placement follows the locks, and no neighbour may end up farther than `high`.
#include <float.h>

#include "common.h"
#include "mesh_select.h"
#include "mesh_tables.h"
#include "stage_timer.h"
#include "../../include/geobi_hip.h"

#pragma clang fp contract(off)

namespace geobi {

namespace {

constexpr int kT = 256;
enum Count { kEdges = 0, kLocked = 1, kValid = 2, kCollapses = 3, kVOut = 4, kFOut = 5, kNotIncluded = 6,
             kSweepsSelected = 7, kCounts = 8 };
static_assert(kCounts <= kSweepBase && kSweepBase + GEOBI_DECIM_SWEEPS <= kDevCounts, "one counter per sweep");
enum Role { kPlain = -1, kMergedAway = 3 };         // 0, 1, 2: the `lo` of a collapsed edge, its placement code

__device__ __forceinline__ double cost_of(const double* q, const P3& p) {
#pragma clang fp contract(off)
  const double diag = ((q[0] * p.x) * p.x + (q[4] * p.y) * p.y) + (q[7] * p.z) * p.z;
  const double off = ((q[1] * p.x) * p.y + (q[2] * p.x) * p.z) + (q[5] * p.y) * p.z;
  const double lin = (q[3] * p.x + q[6] * p.y) + q[8] * p.z;
  return (diag + 2.0 * off) + (2.0 * lin + q[9]);
}

// ---- values
// Q_v over the corner run of v, ascending face id
__global__ void decim_quadrics_kernel(const float* __restrict__ points, const int* __restrict__ fv, int V,
                                      const uint64_t* __restrict__ corners, int n, const int* __restrict__ locked,
                                      double* __restrict__ Q, int* __restrict__ counts) {
#pragma clang fp contract(off)
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  bool is_locked = false;
  if (v < V) {
    is_locked = locked[v] != 0;
    double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = lower_bound(corners, n, (uint64_t)v << 24); j < n && owner_of(corners[j]) == v; ++j) {
      const int f = item_of(corners[j]);
      const P3 a = point_of(points, fv[3 * (size_t)f]), b = point_of(points, fv[3 * (size_t)f + 1]),
               c = point_of(points, fv[3 * (size_t)f + 2]);
      P3 nrm;
      const double s = normal_of(a, b, c, nrm);
      if (s == 0.0) continue;
      const double l = __dsqrt_rn(s);
      const double d = -((nrm.x * a.x + nrm.y * a.y) + nrm.z * a.z);
      const double p[4] = {nrm.x, nrm.y, nrm.z, d};
      int e = 0;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int t = r; t < 4; ++t) {
          q[e] = q[e] + __ddiv_rn(p[r] * p[t], l);
          ++e;
        }
    }
    for (int e = 0; e < 10; ++e) Q[10 * (size_t)v + e] = q[e];
  }
  count_lanes(is_locked, counts + kLocked);
}

// per sorted position: the head of an edge with two claimants whose ends are not both locked takes its placement and runs
// the tests; cost_key = the orderable cost of a valid candidate (else kNoCandidate), hash, code, idx = the position itself
__global__ void decim_candidates_kernel(const uint64_t* __restrict__ keys, int n, const float* __restrict__ points,
                                        const int* __restrict__ fv, const uint64_t* __restrict__ corners,
                                        const uint64_t* __restrict__ pairs, int n_pairs, const int* __restrict__ locked,
                                        const double* __restrict__ Q, int use_max_cost, double max_cost,
                                        uint64_t* __restrict__ cost_key, uint32_t* __restrict__ hash,
                                        int* __restrict__ code_out, int* __restrict__ idx, int* __restrict__ counts) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool valid = false;
  if (i < n) {
    const Run r = run_at(keys, n, i);
    uint64_t ck = kNoCandidate;
    int code = 0;
    const int lo = edge_key_lo(keys[i]), hi = edge_key_hi(keys[i]);      // meaningful at a head
    if (r.head && r.two && !r.three && !(locked[lo] != 0 && locked[hi] != 0)) {
      double q[10];
      for (int e = 0; e < 10; ++e) q[e] = Q[10 * (size_t)lo + e] + Q[10 * (size_t)hi + e];
      const float* pl = points + 3 * (size_t)lo;
      const float* ph = points + 3 * (size_t)hi;
      const P3 place[3] = {point_of(points, lo), point_of(points, hi),
                           {(double)midpoint(pl[0], ph[0]), (double)midpoint(pl[1], ph[1]), (double)midpoint(pl[2], ph[2])}};
      const int first = locked[hi] != 0 ? 1 : 0, last = locked[lo] != 0 ? 0 : (locked[hi] != 0 ? 1 : 2);
      double cost = cost_of(q, place[first]);
      code = first;
      for (int c = first + 1; c <= last; ++c) {
        const double value = cost_of(q, place[c]);
        if (value < cost) { cost = value; code = c; }
      }
      valid = isfinite(cost) && !(use_max_cost != 0 && cost > max_cost);
      if (valid) valid = link_and_valence(pairs, n_pairs, lo, hi);
      if (valid) valid = no_flip(points, fv, corners, n, lo, hi, place[code]);
      if (valid) valid = no_flip(points, fv, corners, n, hi, lo, place[code]);
      if (valid) {
        const uint64_t bits = (uint64_t)__double_as_longlong(cost);
        ck = (bits >> 63) != 0 ? ~bits : bits | (1ull << 63);
      }
    }
    cost_key[i] = ck;
    hash[i] = valid ? (uint32_t)((keys[i] * 0x9E3779B97F4A7C15ull) >> 32) : 0xffffffffu;
    code_out[i] = code;
    idx[i] = i;
  }
  count_lanes(valid, counts + kValid);
}

// ---- the short-edge collapse of 4p: the caller's lock flags join the unit's own; the locked vertices are counted here
// (no quadrics are summed)
__global__ void decim_join_lock_kernel(const int* __restrict__ lock, int V, int* __restrict__ locked,
                                       int* __restrict__ counts) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  bool is_locked = false;
  if (v < V) {
    is_locked = locked[v] != 0 || (lock != nullptr && lock[v] != 0);
    locked[v] = is_locked ? 1 : 0;
  }
  count_lanes(is_locked, counts + kLocked);
}

// no neighbour of v other than lo and hi lies farther than `high` from the placement (squared lengths, ascending id)
__device__ __forceinline__ bool within_high(const float* __restrict__ points, const uint64_t* __restrict__ pairs,
                                            int n_pairs, int v, int lo, int hi, const P3& at, double high2) {
#pragma clang fp contract(off)
  bool ok = true;
  for (int j = lower_bound(pairs, n_pairs, (uint64_t)v << 24); j < n_pairs && owner_of(pairs[j]) == v; ++j) {
    const int w = item_of(pairs[j]);
    if (w == lo || w == hi) continue;
    const P3 p = point_of(points, w);
    const double dx = p.x - at.x, dy = p.y - at.y, dz = p.z - at.z;
    if ((dx * dx + dy * dy) + dz * dz > high2) ok = false;
  }
  return ok;
}

// the candidate kernel of geobi_decim_plan_short: the cost is the squared length, the placement is decided by the locks
__global__ void decim_short_candidates_kernel(const uint64_t* __restrict__ keys, int n, const float* __restrict__ points,
                                              const int* __restrict__ fv, const uint64_t* __restrict__ corners,
                                              const uint64_t* __restrict__ pairs, int n_pairs,
                                              const int* __restrict__ locked, double low2, double high2,
                                              uint64_t* __restrict__ cost_key, uint32_t* __restrict__ hash,
                                              int* __restrict__ code_out, int* __restrict__ idx, int* __restrict__ counts) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool valid = false;
  if (i < n) {
    const Run r = run_at(keys, n, i);
    uint64_t ck = kNoCandidate;
    int code = 0;
    const int lo = edge_key_lo(keys[i]), hi = edge_key_hi(keys[i]);      // meaningful at a head
    if (r.head && r.two && !r.three && !(locked[lo] != 0 && locked[hi] != 0)) {
      const float* pl = points + 3 * (size_t)lo;
      const float* ph = points + 3 * (size_t)hi;
      const double len2 = edge_len2(points, lo, hi);
      code = locked[lo] != 0 ? 0 : (locked[hi] != 0 ? 1 : 2);
      const P3 at = code == 0 ? point_of(points, lo) : code == 1 ? point_of(points, hi) :
                    P3{(double)midpoint(pl[0], ph[0]), (double)midpoint(pl[1], ph[1]), (double)midpoint(pl[2], ph[2])};
      valid = len2 < low2;
      if (valid) valid = within_high(points, pairs, n_pairs, lo, lo, hi, at, high2);
      if (valid) valid = within_high(points, pairs, n_pairs, hi, lo, hi, at, high2);
      if (valid) valid = link_and_valence(pairs, n_pairs, lo, hi);
      if (valid) valid = no_flip(points, fv, corners, n, lo, hi, at);
      if (valid) valid = no_flip(points, fv, corners, n, hi, lo, at);
      if (valid) ck = (uint64_t)__double_as_longlong(len2) | (1ull << 63);          // len2 >= 0: orderable as in 4o
    }
    cost_key[i] = ck;
    hash[i] = valid ? (uint32_t)((keys[i] * 0x9E3779B97F4A7C15ull) >> 32) : 0xffffffffu;
    code_out[i] = code;
    idx[i] = i;
  }
  count_lanes(valid, counts + kValid);
}

__global__ void decim_gather_cost_kernel(const uint64_t* __restrict__ cost_key, const int* __restrict__ idx, int n,
                                         uint64_t* __restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int i = idx[j];
  out[j] = (unsigned)i < (unsigned)n ? cost_key[i] : kNoCandidate;
}

// ---- selection (mesh_select.h): the footprint of a collapse is the two ends of its edge; nothing else is recorded
struct EdgeEnds {
  static constexpr int kSize = 2;
  const uint64_t* keys;
  __device__ void footprint(int i, int* v) const { v[0] = edge_key_lo(keys[i]); v[1] = edge_key_hi(keys[i]); }
  __device__ void record(int) const {}
};

// ---- budget
__global__ void decim_selected_in_rank_order_kernel(const int* __restrict__ order, const int* __restrict__ state, int n,
                                                    int* __restrict__ flag) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int i = order[j];
  flag[j] = (unsigned)i < (unsigned)n && (state[i] & kSelected) != 0 ? 1 : 0;
}

// the first k selected edges in rank order collapse: the roles of their ends, their two claimants go
__global__ void decim_collapse_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ vals, int n,
                                      const int* __restrict__ order, const int* __restrict__ flag,
                                      const int* __restrict__ pos, const int* __restrict__ code, int F, int budget,
                                      int* __restrict__ role, int* __restrict__ partner, int* __restrict__ fkeep,
                                      int* __restrict__ counts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  bool collapses = false;
  if (j < n && flag[j] != 0) {
    const int over = F - counts[kNotIncluded] - budget;            // counts[kNotIncluded]: written by an earlier launch
    const int k = budget < 0 ? n : (over > 0 ? (over + 1) / 2 : 0);
    const int i = order[j];
    if (pos[j] < k && i + 1 < n) {
      collapses = true;
      const int lo = edge_key_lo(keys[i]), hi = edge_key_hi(keys[i]);
      role[lo] = code[i];
      partner[lo] = hi;
      role[hi] = kMergedAway;
      partner[hi] = lo;
      fkeep[(vals[i] >> 1) / 3] = 0;
      fkeep[(vals[i + 1] >> 1) / 3] = 0;
    }
  }
  count_lanes(collapses, counts + kCollapses);
}

__global__ void decim_keep_vertices_kernel(const int* __restrict__ role, int V, int* __restrict__ keep) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < V) keep[v] = role[v] != kMergedAway ? 1 : 0;
}

__global__ void decim_totals_kernel(const int* __restrict__ keepv, const int* __restrict__ vrow, int V,
                                    const int* __restrict__ fkeep, const int* __restrict__ frow, int F,
                                    int* __restrict__ counts) {
  counts[kVOut] = V > 0 ? vrow[V - 1] + keepv[V - 1] : 0;
  counts[kFOut] = frow[F - 1] + fkeep[F - 1];
  int sweeps = 0;
  for (int s = 0; s < GEOBI_DECIM_SWEEPS; ++s) sweeps += counts[kSweepBase + s] > 0 ? 1 : 0;
  counts[kSweepsSelected] = sweeps;
}

__global__ void decim_no_faces_kernel(int V, int* __restrict__ counts) { counts[kVOut] = V; }

// ---- emit
__global__ void decim_vertices_kernel(const int* __restrict__ role, const int* __restrict__ partner,
                                      const int* __restrict__ vrow, int V, int Vn, int* __restrict__ vertex_map,
                                      int* __restrict__ parents, int8_t* __restrict__ place) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const int r = role[v], p = partner[v];
  const bool has_partner = r != kPlain && (unsigned)p < (unsigned)V;
  if (r == kMergedAway && has_partner) {
    vertex_map[v] = vrow[p];
    return;
  }
  const int row = vrow[v];
  vertex_map[v] = row;
  if ((unsigned)row >= (unsigned)Vn) return;
  parents[2 * (size_t)row] = v;
  parents[2 * (size_t)row + 1] = has_partner ? p : v;
  place[row] = (int8_t)(has_partner ? r : 0);
}

// with no plan (F == 0): every row stays
__global__ void decim_identity_kernel(int V, int* __restrict__ vertex_map, int* __restrict__ parents,
                                      int8_t* __restrict__ place) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  vertex_map[v] = v;
  parents[2 * (size_t)v] = v;
  parents[2 * (size_t)v + 1] = v;
  place[v] = 0;
}

__global__ void decim_faces_kernel(const int* __restrict__ fv, int F, int V, const int* __restrict__ fkeep,
                                   const int* __restrict__ frow, const int* __restrict__ role,
                                   const int* __restrict__ partner, const int* __restrict__ vrow, int Fn,
                                   int* __restrict__ faces_out, int* __restrict__ face_map) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F || fkeep[f] == 0) return;
  const int row = frow[f];
  if ((unsigned)row >= (unsigned)Fn) return;
  for (int k = 0; k < 3; ++k) {
    int c = fv[3 * (size_t)f + k];                                  // below V: a kept face is an included one
    if ((unsigned)c >= (unsigned)V) c = 0;                          // never, unless the faces are not those of the plan
    const int p = partner[c];
    const int from = role[c] == kMergedAway && (unsigned)p < (unsigned)V ? p : c;
    faces_out[3 * (size_t)row + k] = vrow[from];
  }
  face_map[row] = f;
}

// one lane per output row: the placement of the row's parents
__global__ void decim_points_kernel(const float* __restrict__ other, int V, int Vn, const int* __restrict__ parents,
                                    const int8_t* __restrict__ place, float* __restrict__ out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= Vn) return;
  const int a = parents[2 * (size_t)r], b = parents[2 * (size_t)r + 1];
  if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V) return;
  const int code = place[r];
  for (int k = 0; k < 3; ++k) {
    const float x = other[3 * (size_t)a + k], y = other[3 * (size_t)b + k];
    out[3 * (size_t)r + k] = code == 0 ? x : (code == 1 ? y : midpoint(x, y));
  }
}

struct DecimBuffers {
  // the state of a plan, read by emit
  int *role, *partner, *vrow, *fkeep, *frow, *counts;
  // scratch of the plan: the three tables
  MeshTables t;
  // per vertex
  double* Q;
  int *locked, *blocked, *m1, *m2, *keepv;
  // per sorted position
  uint64_t *cost_key, *cost_in, *cost_out;
  uint32_t *hash_in, *hash_out;
  int *idx_in, *idx_mid, *order, *code, *rank, *state, *flag, *pos;
  PairSort<uint32_t, int> hash_sort; PairSort<uint64_t, int> cost_sort;
  ExclusiveScan<int> slot_scan, vertex_scan, face_scan;
};
DecimBuffers carve_decim(Arena& a, int64_t F, int64_t V) {
  const int64_t n = 3 * F;
  return {a.take<int>(V), a.take<int>(V), a.take<int>(V), a.take<int>(F), a.take<int>(F), a.take<int>(kDevCounts),
          carve_tables<true, true>(a, F),
          a.take<double>(10 * V),
          a.take<int>(V), a.take<int>(V), a.take<int>(V), a.take<int>(V), a.take<int>(V),
          a.take<uint64_t>(n), a.take<uint64_t>(n), a.take<uint64_t>(n),
          a.take<uint32_t>(n), a.take<uint32_t>(n),
          a.take<int>(n), a.take<int>(n), a.take<int>(n), a.take<int>(n), a.take<int>(n), a.take<int>(n), a.take<int>(n),
          a.take<int>(n),
          PairSort<uint32_t, int>::take(a, n, 32), PairSort<uint64_t, int>::take(a, n, 64),
          ExclusiveScan<int>::take(a, n), ExclusiveScan<int>::take(a, V), ExclusiveScan<int>::take(a, F)};
}

int launch_points(const float* other, int64_t V, int64_t Vn, const int32_t* parents, const int8_t* place, float* out,
                  hipStream_t s) {
  if (Vn == 0) return 0;
  decim_points_kernel<<<cdiv(Vn, kT), kT, 0, s>>>(other, (int)V, (int)Vn, parents, place, out);
  GEOBI_LAUNCH_OK();
  return 0;
}

// one plan: the quadric costs of 4o, or with `sh` the squared lengths of the short-edge collapse of 4p; every kernel but
// the candidate kernel (and the quadric sums it needs) is shared
struct ShortEdges { const int* lock; float low, high; };
int plan_round(const char* what, const int32_t* faces, const float* points, int64_t F, int64_t V, int use_max_cost,
               float max_cost, int64_t budget, const ShortEdges* sh, int32_t* counts, float* stage_ms, void* ws,
               size_t ws_bytes, hipStream_t s) {
  if (F == 0) {                                   // nothing to collapse: V' = V, F' = 0
    GEOBI_HIP(hipMemsetAsync(counts, 0, sizeof(int) * kCounts, s));
    decim_no_faces_kernel<<<1, 1, 0, s>>>((int)V, counts);
    GEOBI_LAUNCH_OK();
    return 0;
  }
  DecimBuffers b;
  GEOBI_TRY(carve_checked(what, ws, ws_bytes, b, [&](Arena& a) { return carve_decim(a, F, V); }));
  const MeshTables& t = b.t;
  const int n = (int)(3 * F), n_pairs = 2 * n;
  const int k_budget = budget < 0 ? -1 : (int)(budget < F ? budget : F);
  StageTimer timer(stage_ms, s);
  GEOBI_TRY(timer.mark());
  // ---- tables
  GEOBI_HIP(hipMemsetAsync(b.counts, 0, sizeof(int) * kDevCounts, s));
  if (V > 0) {
    GEOBI_HIP(hipMemsetAsync(b.locked, 0, sizeof(int) * (size_t)V, s));
    GEOBI_HIP(hipMemsetAsync(b.blocked, 0, sizeof(int) * (size_t)V, s));
    GEOBI_HIP(hipMemsetAsync(b.role, 0xff, sizeof(int) * (size_t)V, s));       // kPlain
    GEOBI_HIP(hipMemsetAsync(b.partner, 0xff, sizeof(int) * (size_t)V, s));
  }
  GEOBI_TRY(build_edge_table(t, faces, nullptr, F, V, s));
  GEOBI_TRY(build_corner_table(t, faces, F, V, b.fkeep, b.counts + kNotIncluded, s));
  GEOBI_TRY(build_pair_table(t, F, b.locked, b.counts + kEdges, s));
  GEOBI_TRY(timer.mark());
  // ---- values and rank
  if (sh != nullptr) {
    if (V > 0) {
      decim_join_lock_kernel<<<cdiv(V, kT), kT, 0, s>>>(sh->lock, (int)V, b.locked, b.counts);
      GEOBI_LAUNCH_OK();
    }
    decim_short_candidates_kernel<<<cdiv(n, kT), kT, 0, s>>>(t.k_out, n, points, faces, t.c_out, t.p_out, n_pairs, b.locked,
                                                            (double)sh->low * (double)sh->low,
                                                            (double)sh->high * (double)sh->high, b.cost_key, b.hash_in,
                                                            b.code, b.idx_in, b.counts);
    GEOBI_LAUNCH_OK();
  } else {
    if (V > 0) {
      decim_quadrics_kernel<<<cdiv(V, kT), kT, 0, s>>>(points, faces, (int)V, t.c_out, n, b.locked, b.Q, b.counts);
      GEOBI_LAUNCH_OK();
    }
    decim_candidates_kernel<<<cdiv(n, kT), kT, 0, s>>>(t.k_out, n, points, faces, t.c_out, t.p_out, n_pairs, b.locked, b.Q,
                                                      use_max_cost, (double)max_cost, b.cost_key, b.hash_in, b.code,
                                                      b.idx_in, b.counts);
    GEOBI_LAUNCH_OK();
  }
  GEOBI_TRY(b.hash_sort.run(b.hash_in, b.hash_out, b.idx_in, b.idx_mid, s));
  decim_gather_cost_kernel<<<cdiv(n, kT), kT, 0, s>>>(b.cost_key, b.idx_mid, n, b.cost_in);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.cost_sort.run(b.cost_in, b.cost_out, b.idx_mid, b.order, s));
  rank_kernel<<<cdiv(n, kT), kT, 0, s>>>(b.cost_out, b.order, n, b.rank, b.state);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(timer.mark());
  // ---- selection
  GEOBI_TRY(run_select_sweeps(EdgeEnds{t.k_out}, GEOBI_DECIM_SWEEPS, n, V, t.p_out, n_pairs, b.rank, b.state, b.m1, b.m2,
                              b.blocked, b.counts + kSweepBase, s));
  // ---- budget, roles, scans
  decim_selected_in_rank_order_kernel<<<cdiv(n, kT), kT, 0, s>>>(b.order, b.state, n, b.flag);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.slot_scan.run(b.flag, b.pos, s));
  decim_collapse_kernel<<<cdiv(n, kT), kT, 0, s>>>(t.k_out, t.v_out, n, b.order, b.flag, b.pos, b.code, (int)F, k_budget,
                                                  b.role, b.partner, b.fkeep, b.counts);
  GEOBI_LAUNCH_OK();
  if (V > 0) {
    decim_keep_vertices_kernel<<<cdiv(V, kT), kT, 0, s>>>(b.role, (int)V, b.keepv);
    GEOBI_LAUNCH_OK();
    GEOBI_TRY(b.vertex_scan.run(b.keepv, b.vrow, s));
  }
  GEOBI_TRY(b.face_scan.run(b.fkeep, b.frow, s));
  decim_totals_kernel<<<1, 1, 0, s>>>(b.keepv, b.vrow, (int)V, b.fkeep, b.frow, (int)F, b.counts);
  GEOBI_LAUNCH_OK();
  GEOBI_HIP(hipMemcpyAsync(counts, b.counts, sizeof(int) * kCounts, hipMemcpyDeviceToDevice, s));
  GEOBI_TRY(timer.mark());
  return timer.finish();
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

size_t geobi_decim_ws_bytes(int64_t F, int64_t V) {
  if (sizes_ok("geobi_decim_ws_bytes", F > V ? F : V, 0) != 0 || (F < V ? F : V) < 0) return 0;
  return carve_bytes([&](Arena& a) { carve_decim(a, F, V); });
}

int geobi_decim_plan(const int32_t* faces, const float* points, int64_t F, int64_t V, int use_max_cost, float max_cost,
                     int64_t budget, int32_t* counts, float* stage_ms, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(points); GEOBI_NOTNULL(counts);
  GEOBI_REQUIRE(use_max_cost == 0 || max_cost >= 0.0f, "decim_plan: max_cost = %g (not negative, not NaN)", (double)max_cost);
  return plan_round("decim_plan", faces, points, F, V, use_max_cost, max_cost, budget, nullptr, counts, stage_ms, ws, ws_bytes,
                    as_stream(stream));
}

int geobi_decim_plan_short(const int32_t* faces, const float* points, const int32_t* lock, int64_t F, int64_t V, float low,
                           float high, int32_t* counts, float* stage_ms, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(points); GEOBI_NOTNULL(counts);
  GEOBI_REQUIRE(low > 0.0f && high >= low && high <= FLT_MAX,
                "decim_plan_short: low = %g, high = %g (0 < low <= high, finite)", (double)low, (double)high);
  const ShortEdges sh = {lock, low, high};
  return plan_round("decim_plan_short", faces, points, F, V, 0, 0.0f, -1, &sh, counts, stage_ms, ws, ws_bytes,
                    as_stream(stream));
}

int geobi_decim_emit(const int32_t* faces, const float* points, int64_t F, int64_t V, int64_t Vn, int64_t Fn,
                     float* points_out, int32_t* faces_out, int32_t* face_map, int32_t* vertex_map,
                     int32_t* vertex_parents, int8_t* place, const void* ws, size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_MESH_SIZES(Vn, Fn);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(points); GEOBI_NOTNULL(points_out); GEOBI_NOTNULL(faces_out);
  GEOBI_NOTNULL(face_map); GEOBI_NOTNULL(vertex_map); GEOBI_NOTNULL(vertex_parents); GEOBI_NOTNULL(place);
  GEOBI_REQUIRE(Vn <= V && Fn <= F && 2 * (V - Vn) <= F - Fn,
                "decim_emit: V' = %lld, F' = %lld are not what a plan of V = %lld, F = %lld can give", (long long)Vn,
                (long long)Fn, (long long)V, (long long)F);
  hipStream_t s = as_stream(stream);
  if (F == 0) {
    if (V > 0) {
      decim_identity_kernel<<<cdiv(V, kT), kT, 0, s>>>((int)V, vertex_map, vertex_parents, place);
      GEOBI_LAUNCH_OK();
    }
    return launch_points(points, V, Vn, vertex_parents, place, points_out, s);
  }
  DecimBuffers b;
  GEOBI_TRY(carve_checked("decim_emit", const_cast<void*>(ws), ws_bytes, b, [&](Arena& a) { return carve_decim(a, F, V); }));
  if (V > 0) {
    decim_vertices_kernel<<<cdiv(V, kT), kT, 0, s>>>(b.role, b.partner, b.vrow, (int)V, (int)Vn, vertex_map, vertex_parents,
                                                    place);
    GEOBI_LAUNCH_OK();
    decim_faces_kernel<<<cdiv(F, kT), kT, 0, s>>>(faces, (int)F, (int)V, b.fkeep, b.frow, b.role, b.partner, b.vrow, (int)Fn,
                                                 faces_out, face_map);
    GEOBI_LAUNCH_OK();
  }
  return launch_points(points, V, Vn, vertex_parents, place, points_out, s);
}

int geobi_decim_points(const float* other, int64_t V, int64_t Vn, const int32_t* vertex_parents, const int8_t* place,
                       float* out, void* stream) {
  GEOBI_MESH_SIZES(V, Vn);
  GEOBI_NOTNULL(other); GEOBI_NOTNULL(vertex_parents); GEOBI_NOTNULL(place); GEOBI_NOTNULL(out);
  GEOBI_REQUIRE(Vn <= V, "decim_points: V' = %lld rows from V = %lld", (long long)Vn, (long long)V);
  return launch_points(other, V, Vn, vertex_parents, place, out, as_stream(stream));
}

}  // extern "C"
