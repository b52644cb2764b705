// Triangle-mesh refinement on the device: midpoint / Loop / max-edge subdivision, one pass per
// plan + emit.  The rules are stated in include/geobi_hip.h (geobi_subdiv_*); tests/subdiv_model.py restates them
// sequentially and every output is compared bit for bit.
//
// The topology is integer-exact and independent of launch geometry; positions go through one stated sequence of
// roundings (contraction off throughout), no float atomics:
//   table    the edge table of edge_table.h (slots and sort called one by one: a timer mark lies between): a run is an
//            edge, the run heads ascend with (lo, hi) -- the sorted position of a head orders the edges as their ids do, so
//            the rank of a split edge among the split edges is the exclusive scan of the split flags of the heads
//   plan     per sorted position: head / boundary / complex / split (counted with count_lanes); scan of the split flags;
//            per slot the rank of its edge's midpoint (or -1); per face 1 + its split edges children, scanned; V', F'.
//            Loop only: every edge head lists its two DIRECTED pairs (src << 24 | dst) << 1 | sharp, sorted on 49 bits --
//            the neighbours of a vertex in ascending id, one binary search away
//   emit     one lane per face (children, face_parent), per vertex (old rows) and per sorted position (new rows)
// Every index is bounded: corners are below V (face_included), slots below 3F, child rows below F' and new rows below V'
// (checked against the sizes the caller read from the plan's counts).
#include "common.h"
#include "edge_table.h"
#include "mesh_rings.h"
#include "stage_timer.h"
#include "../../include/geobi_hip.h"

namespace geobi {

namespace {

constexpr int kT = 256;
enum Count { kEdges = 0, kSplit = 1, kBoundary = 2, kComplex = 3, kVOut = 4, kFOut = 5, kHasLoop = 6, kCounts = 8 };
constexpr unsigned kPairBits = kEdgeKeyBits + 1;               // a directed pair: (src << 24 | dst) << 1 | sharp
constexpr uint64_t kNoPair = (1ull << kPairBits) - 1;          // sorts last; its src field is 2^24 - 1, never a vertex

// uniform: every edge; adaptive: strictly longer than L
__device__ __forceinline__ bool edge_is_split(const float* __restrict__ points, uint64_t key, int adaptive, double L2) {
  return adaptive == 0 || edge_len2(points, edge_key_lo(key), edge_key_hi(key)) > L2;
}

// per sorted position: split[i] = 1 at the head of a split edge, else 0; counts of edges, split, boundary, complex edges
__global__ void subdiv_flags_kernel(const uint64_t* __restrict__ keys, int n, const float* __restrict__ points,
                                    int adaptive, double L2, int* __restrict__ split, int* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool head = false, boundary = false, complex_edge = false, is_split = false;
  if (i < n) {
    const uint64_t key = keys[i];
    head = key != kNoEdge && (i == 0 || keys[i - 1] != key);
    if (head) {
      const bool two = i + 1 < n && keys[i + 1] == key, three = two && i + 2 < n && keys[i + 2] == key;
      boundary = !two;
      complex_edge = three;
      is_split = edge_is_split(points, key, adaptive, L2);
    }
    split[i] = is_split ? 1 : 0;
  }
  count_lanes(head, counts + kEdges);
  count_lanes(is_split, counts + kSplit);
  count_lanes(boundary, counts + kBoundary);
  count_lanes(complex_edge, counts + kComplex);
}

// slot_mid[slot] = the rank of the slot's edge among the split edges, -1 when it is not split (or the face not included).
// rank = the exclusive scan of split: at a head its own rank, at a later claimant of a split edge one more
__global__ void subdiv_slot_mid_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ vals, int n,
                                       const float* __restrict__ points, int adaptive, double L2,
                                       const int* __restrict__ split, const int* __restrict__ rank,
                                       int* __restrict__ slot_mid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  int m = -1;
  if (key != kNoEdge) {
    const bool head = i == 0 || keys[i - 1] != key;
    const bool is_split = head ? split[i] != 0 : edge_is_split(points, key, adaptive, L2);
    if (is_split) m = head ? rank[i] : rank[i] - 1;
  }
  slot_mid[vals[i] >> 1] = m;
}

__global__ void subdiv_child_count_kernel(const int* __restrict__ slot_mid, int F, int* __restrict__ children) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  children[f] = 1 + (slot_mid[3 * (size_t)f] >= 0) + (slot_mid[3 * (size_t)f + 1] >= 0) + (slot_mid[3 * (size_t)f + 2] >= 0);
}

__global__ void subdiv_totals_kernel(const int* __restrict__ children, const int* __restrict__ first_child, int F, int V,
                                     int loop, int* __restrict__ counts) {
  counts[kVOut] = V + counts[kSplit];
  counts[kFOut] = first_child[F - 1] + children[F - 1];
  counts[kHasLoop] = loop;
}

__global__ void subdiv_no_faces_kernel(int V, int* __restrict__ counts) { counts[kVOut] = V; }

// Loop: the two directed pairs of every edge, at 2i and 2i + 1 of its head's sorted position; sharp = not exactly two claimants
__global__ void subdiv_pairs_kernel(const uint64_t* __restrict__ keys, int n, uint64_t* __restrict__ pairs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  uint64_t forth = kNoPair, back = kNoPair;
  if (key != kNoEdge && (i == 0 || keys[i - 1] != key)) {
    const bool two = i + 1 < n && keys[i + 1] == key, three = two && i + 2 < n && keys[i + 2] == key;
    const uint64_t sharp = two && !three ? 0 : 1;
    forth = key << 1 | sharp;
    back = edge_key(edge_key_hi(key), edge_key_lo(key)) << 1 | sharp;
  }
  pairs[2 * (size_t)i] = forth;
  pairs[2 * (size_t)i + 1] = back;
}

// the far end of a directed pair, as an index (edge_table.h: index_from_key)
__device__ __forceinline__ int pair_end(uint64_t pair) { return index_from_key((int)(pair >> 1 & 0xffffffull)); }

// ---- emit
struct Child { int a, b, c; };

// the children of every face in the order of the header, face_parent = the face
__global__ void subdiv_faces_kernel(const int* __restrict__ fv, int F, int V, const float* __restrict__ points,
                                    const int* __restrict__ slot_mid, const int* __restrict__ first_child, int Fn,
                                    int* __restrict__ faces_out, int* __restrict__ face_parent) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const int c0 = fv[3 * (size_t)f], c1 = fv[3 * (size_t)f + 1], c2 = fv[3 * (size_t)f + 2];
  const int r0 = slot_mid[3 * (size_t)f], r1 = slot_mid[3 * (size_t)f + 1], r2 = slot_mid[3 * (size_t)f + 2];
  const int m0 = V + r0, m1 = V + r1, m2 = V + r2;                 // meaningful where r >= 0
  const int n_split = (r0 >= 0) + (r1 >= 0) + (r2 >= 0);
  Child ch[4];
  if (n_split == 0) {
    ch[0] = {c0, c1, c2};
  } else if (n_split == 3) {
    ch[0] = {c0, m0, m2}; ch[1] = {c1, m1, m0}; ch[2] = {c2, m2, m1}; ch[3] = {m0, m1, m2};
  } else if (n_split == 1) {                                        // edge k: a = c_k, b = c_k+1, c = c_k+2
    const int a = r0 >= 0 ? c0 : (r1 >= 0 ? c1 : c2), b = r0 >= 0 ? c1 : (r1 >= 0 ? c2 : c0),
              c = r0 >= 0 ? c2 : (r1 >= 0 ? c0 : c1), m = r0 >= 0 ? m0 : (r1 >= 0 ? m1 : m2);
    ch[0] = {a, m, c}; ch[1] = {m, b, c};
  } else {                                                          // edge u unsplit: a = c_u, b = c_u+1, c = c_u+2
    const int a = r0 < 0 ? c0 : (r1 < 0 ? c1 : c2), b = r0 < 0 ? c1 : (r1 < 0 ? c2 : c0),
              c = r0 < 0 ? c2 : (r1 < 0 ? c0 : c1);
    const int p = r0 < 0 ? m1 : (r1 < 0 ? m2 : m0), q = r0 < 0 ? m2 : (r1 < 0 ? m0 : m1);   // on b - c and on c - a
    const int lo1 = b < c ? b : c, hi1 = b < c ? c : b, lo2 = c < a ? c : a, hi2 = c < a ? a : c;
    const double l1 = edge_len2(points, lo1, hi1), l2 = edge_len2(points, lo2, hi2);
    // edge ids ascend with the keys: the tie goes to the lower key
    const bool first_longer = l1 > l2 || (l1 == l2 && edge_key(lo1, hi1) < edge_key(lo2, hi2));
    ch[0] = {p, c, q};
    if (first_longer) { ch[1] = {a, b, p}; ch[2] = {a, p, q}; }
    else { ch[1] = {a, b, q}; ch[2] = {b, p, q}; }
  }
  const int first = first_child[f];
  for (int k = 0; k <= n_split; ++k) {
    const int row = first + k;
    if (row < 0 || row >= Fn) continue;
    faces_out[3 * (size_t)row] = ch[k].a;
    faces_out[3 * (size_t)row + 1] = ch[k].b;
    faces_out[3 * (size_t)row + 2] = ch[k].c;
    face_parent[row] = f;
  }
}

__global__ void subdiv_old_parents_kernel(int V, int* __restrict__ parents) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  parents[2 * (size_t)v] = v;
  parents[2 * (size_t)v + 1] = v;
}

__global__ void subdiv_new_parents_kernel(const uint64_t* __restrict__ keys, int n, const int* __restrict__ split,
                                          const int* __restrict__ rank, int V, int Vn, int* __restrict__ parents) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || split[i] == 0) return;
  const int row = V + rank[i];
  if (row < V || row >= Vn) return;
  parents[2 * (size_t)row] = edge_key_lo(keys[i]);
  parents[2 * (size_t)row + 1] = edge_key_hi(keys[i]);
}

// the rows V .. V' - 1: one lane per sorted position, the heads of split edges write.  Loop: an edge with exactly two
// claimants takes 3/8 (lo + hi) + 1/8 (c + d) in fp64, c and d the opposite corners of its two claimants
__global__ void subdiv_new_points_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ vals, int n,
                                         const int* __restrict__ fv, const int* __restrict__ split,
                                         const int* __restrict__ rank, const float* __restrict__ points, int V, int Vn,
                                         int loop, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || split[i] == 0) return;
  const int row = V + rank[i];
  if (row < V || row >= Vn) return;
  const uint64_t key = keys[i];
  const size_t lo = 3 * (size_t)edge_key_lo(key), hi = 3 * (size_t)edge_key_hi(key);
  const bool two = i + 1 < n && keys[i + 1] == key, three = two && i + 2 < n && keys[i + 2] == key;
  if (loop != 0 && two && !three) {
    const int s0 = vals[i] >> 1, s1 = vals[i + 1] >> 1;
    const size_t c = 3 * (size_t)fv[3 * (size_t)(s0 / 3) + (s0 % 3 + 2) % 3];
    const size_t d = 3 * (size_t)fv[3 * (size_t)(s1 / 3) + (s1 % 3 + 2) % 3];
    for (int k = 0; k < 3; ++k) {
      const double ends = (double)points[lo + k] + (double)points[hi + k];
      const double wings = (double)points[c + k] + (double)points[d + k];
      out[3 * (size_t)row + k] = (float)(0.375 * ends + 0.125 * wings);
    }
  } else {
    for (int k = 0; k < 3; ++k) out[3 * (size_t)row + k] = midpoint(points[lo + k], points[hi + k]);
  }
}

__global__ void subdiv_copy_points_kernel(const float* __restrict__ points, int n, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = points[i];
}

// Loop, the rows 0 .. V - 1: one lane per vertex walks its directed pairs, which list its neighbours in ascending id
__global__ void subdiv_loop_even_kernel(const float* __restrict__ points, int V, const uint64_t* __restrict__ pairs,
                                        int n_pairs, const int* __restrict__ counts, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const float own[3] = {points[3 * (size_t)v], points[3 * (size_t)v + 1], points[3 * (size_t)v + 2]};
  int begin = 0, n = 0, n_sharp = 0, sharp_end[2] = {0, 0};
  if (counts[kHasLoop] != 0) {                    // a plan made for the midpoint scheme has no pairs: every row unchanged
    const uint64_t first = (uint64_t)v << (kPairBits - 24);
    int lo = 0, hi = n_pairs;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (pairs[mid] < first) lo = mid + 1; else hi = mid;
    }
    begin = lo;
    for (int j = begin; j < n_pairs && (int)(pairs[j] >> (kPairBits - 24)) == v; ++j) {
      if ((pairs[j] & 1) != 0) {
        if (n_sharp < 2) sharp_end[n_sharp] = pair_end(pairs[j]);
        ++n_sharp;
      }
      ++n;
    }
  }
  double result[3] = {0.0, 0.0, 0.0};
  bool moved = false;
  if (n_sharp == 0 && n >= 1) {
    const double beta = n == 3 ? 3.0 / 16.0 : 3.0 / (8.0 * (double)n);
    const double keep = 1.0 - (double)n * beta;
    double sum[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < n; ++j) {
      const int w = pair_end(pairs[begin + j]);
      if (w >= V) continue;                       // never: the pairs come from corners below V
      for (int k = 0; k < 3; ++k) {
        const double x = (double)points[3 * (size_t)w + k];
        sum[k] = j == 0 ? x : sum[k] + x;
      }
    }
    for (int k = 0; k < 3; ++k) result[k] = keep * (double)own[k] + beta * sum[k];
    moved = true;
  } else if (n_sharp == 2 && sharp_end[0] < V && sharp_end[1] < V) {
    for (int k = 0; k < 3; ++k) {
      const double ends = (double)points[3 * (size_t)sharp_end[0] + k] + (double)points[3 * (size_t)sharp_end[1] + k];
      result[k] = 0.75 * (double)own[k] + 0.125 * ends;
    }
    moved = true;
  }
  for (int k = 0; k < 3; ++k) out[3 * (size_t)v + k] = moved ? (float)result[k] : own[k];
}

struct SubdivBuffers {
  // the state of a plan, read by emit and points: the sorted edge table (t.k_out, t.v_out) and
  MeshTables t;
  int *split, *rank, *slot_mid, *first_child, *counts;
  uint64_t* p_out;                 // Loop: the sorted 49-bit pairs (not the pair table of mesh_tables.h)
  // scratch of the plan
  uint64_t* p_in;
  int* children;
  KeySort<uint64_t> pair_sort; ExclusiveScan<int> slot_scan, face_scan;
};
SubdivBuffers carve_subdiv(Arena& a, int64_t F) {
  return {carve_tables<false, false>(a, F),
          a.take<int>(3 * F), a.take<int>(3 * F), a.take<int>(3 * F), a.take<int>(F), a.take<int>(kCounts),
          a.take<uint64_t>(6 * F),
          a.take<uint64_t>(6 * F), a.take<int>(F),
          KeySort<uint64_t>::take(a, 6 * F, kPairBits), ExclusiveScan<int>::take(a, 3 * F), ExclusiveScan<int>::take(a, F)};
}

int subdiv_buffers(const char* what, int64_t F, void* ws, size_t ws_bytes, SubdivBuffers& b) {
  return carve_checked(what, ws, ws_bytes, b, [&](Arena& a) { return carve_subdiv(a, F); });
}

// the rows of points_out [Vn, 3] from points [V, 3] over the plan in b
int launch_points(const int32_t* faces, const float* points, int64_t F, int64_t V, int loop, int64_t Vn,
                  const SubdivBuffers& b, float* points_out, hipStream_t s) {
  if (V > 0) {
    if (loop != 0)
      subdiv_loop_even_kernel<<<cdiv(V, kT), kT, 0, s>>>(points, (int)V, b.p_out, (int)(6 * F), b.counts, points_out);
    else
      subdiv_copy_points_kernel<<<cdiv(3 * V, kT), kT, 0, s>>>(points, (int)(3 * V), points_out);
    GEOBI_LAUNCH_OK();
  }
  subdiv_new_points_kernel<<<cdiv(3 * F, kT), kT, 0, s>>>(b.t.k_out, b.t.v_out, (int)(3 * F), faces, b.split, b.rank, points,
                                                         (int)V, (int)Vn, loop, points_out);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

size_t geobi_subdiv_ws_bytes(int64_t F, int64_t V) {
  if (sizes_ok("geobi_subdiv_ws_bytes", F > V ? F : V, 0) != 0 || (F < V ? F : V) < 0) return 0;
  return carve_bytes([&](Arena& a) { carve_subdiv(a, F); });
}

int geobi_subdiv_plan(const int32_t* faces, const float* points, int64_t F, int64_t V, int loop, int adaptive,
                      float max_edge, int32_t* counts, float* stage_ms, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(counts);
  GEOBI_REQUIRE(!(loop != 0 && adaptive != 0), "subdiv_plan: the Loop scheme has no max_edge mode");
  if (adaptive != 0) {
    GEOBI_NOTNULL(points);
    GEOBI_REQUIRE(max_edge > 0.0f && max_edge < INFINITY, "subdiv_plan: max_edge = %g (positive and finite)", (double)max_edge);
  }
  hipStream_t s = as_stream(stream);
  if (F == 0) {                                   // nothing to split: V' = V, F' = 0
    GEOBI_HIP(hipMemsetAsync(counts, 0, sizeof(int) * kCounts, s));
    subdiv_no_faces_kernel<<<1, 1, 0, s>>>((int)V, counts);
    GEOBI_LAUNCH_OK();
    return 0;
  }
  SubdivBuffers b;
  GEOBI_TRY(subdiv_buffers("subdiv_plan", F, ws, ws_bytes, b));
  const int n = (int)(3 * F);
  const double L2 = (double)max_edge * (double)max_edge;
  StageTimer timer(stage_ms, s);
  GEOBI_TRY(timer.mark());
  edge_slots_kernel<<<cdiv(F, kT), kT, 0, s>>>(faces, nullptr, (int)F, (int)V, b.t.k_in, b.t.v_in);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(timer.mark());
  GEOBI_TRY(sort_edge_table(b.t, F, s));
  GEOBI_TRY(timer.mark());
  GEOBI_HIP(hipMemsetAsync(b.counts, 0, sizeof(int) * kCounts, s));
  subdiv_flags_kernel<<<cdiv(n, kT), kT, 0, s>>>(b.t.k_out, n, points, adaptive, L2, b.split, b.counts);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.slot_scan.run(b.split, b.rank, s));
  subdiv_slot_mid_kernel<<<cdiv(n, kT), kT, 0, s>>>(b.t.k_out, b.t.v_out, n, points, adaptive, L2, b.split, b.rank, b.slot_mid);
  GEOBI_LAUNCH_OK();
  subdiv_child_count_kernel<<<cdiv(F, kT), kT, 0, s>>>(b.slot_mid, (int)F, b.children);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.face_scan.run(b.children, b.first_child, s));
  subdiv_totals_kernel<<<1, 1, 0, s>>>(b.children, b.first_child, (int)F, (int)V, loop != 0 ? 1 : 0, b.counts);
  GEOBI_LAUNCH_OK();
  if (loop != 0) {
    subdiv_pairs_kernel<<<cdiv(n, kT), kT, 0, s>>>(b.t.k_out, n, b.p_in);
    GEOBI_LAUNCH_OK();
    GEOBI_TRY(b.pair_sort.run(b.p_in, b.p_out, s));
  }
  GEOBI_HIP(hipMemcpyAsync(counts, b.counts, sizeof(int) * kCounts, hipMemcpyDeviceToDevice, s));
  GEOBI_TRY(timer.mark());
  return timer.finish();
}

int geobi_subdiv_emit(const int32_t* faces, const float* points, int64_t F, int64_t V, int loop, int64_t Vn, int64_t Fn,
                      int32_t* faces_out, int32_t* face_parent, int32_t* vertex_parents, float* points_out,
                      const void* ws, size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_SIZES(Vn > Fn ? Vn : Fn, 0);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(points); GEOBI_NOTNULL(faces_out); GEOBI_NOTNULL(face_parent);
  GEOBI_NOTNULL(vertex_parents); GEOBI_NOTNULL(points_out);
  GEOBI_REQUIRE(Vn >= V && Fn >= F && Fn <= 4 * F && Vn - V <= 3 * F,
                "subdiv_emit: V' = %lld, F' = %lld are not what a plan of V = %lld, F = %lld can give", (long long)Vn,
                (long long)Fn, (long long)V, (long long)F);
  hipStream_t s = as_stream(stream);
  if (V > 0) {
    subdiv_old_parents_kernel<<<cdiv(V, kT), kT, 0, s>>>((int)V, vertex_parents);
    GEOBI_LAUNCH_OK();
  }
  if (F == 0) {
    if (V > 0) GEOBI_HIP(hipMemcpyAsync(points_out, points, sizeof(float) * 3 * (size_t)V, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  SubdivBuffers b;
  GEOBI_TRY(subdiv_buffers("subdiv_emit", F, const_cast<void*>(ws), ws_bytes, b));
  subdiv_faces_kernel<<<cdiv(F, kT), kT, 0, s>>>(faces, (int)F, (int)V, points, b.slot_mid, b.first_child, (int)Fn, faces_out,
                                                 face_parent);
  GEOBI_LAUNCH_OK();
  subdiv_new_parents_kernel<<<cdiv(3 * F, kT), kT, 0, s>>>(b.t.k_out, (int)(3 * F), b.split, b.rank, (int)V, (int)Vn,
                                                          vertex_parents);
  GEOBI_LAUNCH_OK();
  return launch_points(faces, points, F, V, loop, Vn, b, points_out, s);
}

int geobi_subdiv_points(const int32_t* faces, const float* points, int64_t F, int64_t V, int loop, int64_t Vn,
                        float* points_out, const void* ws, size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_SIZES(Vn, 0);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(points); GEOBI_NOTNULL(points_out);
  GEOBI_REQUIRE(Vn >= V && Vn - V <= 3 * F, "subdiv_points: V' = %lld is not what a plan of V = %lld, F = %lld can give",
                (long long)Vn, (long long)V, (long long)F);
  hipStream_t s = as_stream(stream);
  if (F == 0) {
    if (V > 0) GEOBI_HIP(hipMemcpyAsync(points_out, points, sizeof(float) * 3 * (size_t)V, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  SubdivBuffers b;
  GEOBI_TRY(subdiv_buffers("subdiv_points", F, const_cast<void*>(ws), ws_bytes, b));
  return launch_points(faces, points, F, V, loop, Vn, b, points_out, s);
}

}  // extern "C"
