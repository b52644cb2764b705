// Isotropic remeshing on the device: the lock flags, the edge flips towards the target valence and
// the tangential relaxation of the split / collapse / flip / relax loop.  The split step is subdiv.hip (max_edge), the
// short-edge collapse is geobi_decim_plan_short of decim.hip.  The rules are stated in include/geobi_hip.h (geobi_remesh_*,
// geobi_flip_*, geobi_relax, geobi_move_to); tests/remesh_model.py restates them sequentially (tests/project_model.py:
// geobi_move_to, the step back onto the input surface of DESIGN.md 4r) and every output is compared bit for bit.
//
// The topology is integer-exact and independent of launch geometry; every float step is fp64 in one stated order
// (contraction off throughout, __ddiv_rn / __dsqrt_rn, no float atomics):
//   tables   those of edge_table.h and mesh_tables.h: the edge table (a run is an edge, known by the sorted position of its
//            head), the directed pairs of the run heads (the neighbours of a vertex in ascending id, its valence their
//            number, "does the edge c - d exist" one binary search), for the relaxation also the corner keys
//   lock     one lane per sorted position: integer atomicOr of the bits into the flags (nobody reads them in that launch)
//   flips    one lane per edge head finds the quad, the gain and the validity; ONE stable 64-bit sort of (16 - gain) << 32 |
//            hash ranks the valid candidates (ties keep the position, which orders as the edge ids do); the sweeps of
//            mesh_select.h over the four quad vertices; a selected lane notes its position at its two faces; emit is one
//            lane per face
//   relax    one lane per vertex proposes and tests its move against the old positions, one lane per face marks the
//            vertices of a face that turned, one lane per vertex takes them back, one lane per face counts what is left;
//            move_to is the same text with the proposal read from an array
// Every index is bounded: corners are below V (face_included), slots below 3F, vertices and faces taken out of a key were
// put into it from such a corner or face, positions noted at a face are checked against 3F before they are used.
#include "common.h"
#include "mesh_select.h"
#include "mesh_tables.h"
#include "stage_timer.h"
#include "../../include/geobi_hip.h"

#pragma clang fp contract(off)

namespace geobi {

namespace {

constexpr int kT = 256;
enum LockCount { kLockEdges = 0, kLockBoundary = 1, kLockSharpEdges = 2, kLockSharp = 3, kLockCounts = 4 };
enum FlipCount { kFlipEdges = 0, kFlipCandidates = 1, kFlipValid = 2, kFlips = 3, kFlipSweeps = 4, kFlipCounts = 5 };
enum RelaxCount { kMoved = 0, kRefused = 1, kReverted = 2, kTurned = 3, kRelaxCounts = 4 };
constexpr int kSpareCount = kDevCounts - 1;          // the edge count of a call that does not report it
static_assert(kFlipCounts <= kSweepBase && kSweepBase + GEOBI_FLIP_SWEEPS <= kSpareCount, "one counter per sweep");

__device__ __forceinline__ int valence_of(const uint64_t* __restrict__ pairs, int n_pairs, int v) {
  return lower_bound(pairs, n_pairs, (uint64_t)(v + 1) << 24) - lower_bound(pairs, n_pairs, (uint64_t)v << 24);
}

// the face of a slot value (slot << 1 | direction), below F: the value was written by edge_slots_kernel
__device__ __forceinline__ int face_of_slot_value(int value, int F) {
  const int f = (value >> 1) / 3;
  return (unsigned)f < (unsigned)F ? f : 0;
}

__device__ __forceinline__ double face_normal(const float* __restrict__ points, const int* __restrict__ fv, int f, P3& n) {
  return normal_of(point_of(points, fv[3 * (size_t)f]), point_of(points, fv[3 * (size_t)f + 1]),
                   point_of(points, fv[3 * (size_t)f + 2]), n);
}

// SHARP: the edge at the sorted positions i, i + 1 (two claimants, in slot order), each normal from its face's own row
__device__ __forceinline__ bool edge_sharp(const float* __restrict__ points, const int* __restrict__ fv,
                                           const int* __restrict__ vals, int i, int F, double c2) {
#pragma clang fp contract(off)
  P3 n0, n1;
  const double s0 = face_normal(points, fv, face_of_slot_value(vals[i], F), n0);
  const double s1 = face_normal(points, fv, face_of_slot_value(vals[i + 1], F), n1);
  if (s0 == 0.0 || s1 == 0.0) return false;
  const double dot = dot_of(n0, n1);
  return !(dot > 0.0) || dot * dot < c2 * (s0 * s1);
}

// ---- lock flags
__global__ void remesh_lock_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ vals, int n,
                                   const float* __restrict__ points, const int* __restrict__ fv, int F, int use_sharp,
                                   double c2, int* __restrict__ lock, int* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool sharp = false;
  if (i < n) {
    const Run r = run_at(keys, n, i);
    if (r.head) {
      const int lo = edge_key_lo(keys[i]), hi = edge_key_hi(keys[i]);
      if (!r.two || r.three) {
        atomicOr(lock + lo, 1);
        atomicOr(lock + hi, 1);
      } else if (use_sharp != 0 && edge_sharp(points, fv, vals, i, F, c2)) {
        sharp = true;
        atomicOr(lock + lo, 2);
        atomicOr(lock + hi, 2);
      }
    }
  }
  count_lanes(sharp, counts + kLockSharpEdges);
}

__global__ void remesh_lock_counts_kernel(const int* __restrict__ lock, int V, int* __restrict__ counts) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const int bits = v < V ? lock[v] : 0;
  count_lanes((bits & 1) != 0, counts + kLockBoundary);
  count_lanes((bits & 2) != 0, counts + kLockSharp);
}

// ---- flips
__device__ __forceinline__ int deviation(int valence, int lock_bits) {
  const int d = valence - ((lock_bits & 1) != 0 ? 4 : 6);
  return d < 0 ? -d : d;
}

// per sorted position: the head of an edge with two claimants that walk it in opposite directions and that is not sharp
// finds its quad (a, b, c, d), its gain and its validity; key = (16 - gain) << 32 | hash of a valid candidate, else
// kNoCandidate
__global__ void flip_candidates_kernel(const uint64_t* __restrict__ keys, const int* __restrict__ vals, int n,
                                       const float* __restrict__ points, const int* __restrict__ fv, int F, int V,
                                       const uint64_t* __restrict__ pairs, int n_pairs, const int* __restrict__ lock,
                                       int use_sharp, double c2, uint64_t* __restrict__ key_out, int* __restrict__ idx,
                                       int* __restrict__ qc, int* __restrict__ qd, int* __restrict__ counts) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool candidate = false, valid = false;
  if (i < n) {
    const Run r = run_at(keys, n, i);
    uint64_t key = kNoCandidate;
    int c = 0, d = 0;
    if (r.head && r.two && !r.three && ((vals[i] ^ vals[i + 1]) & 1) != 0) {
      const int a = edge_key_lo(keys[i]), b = edge_key_hi(keys[i]);
      const int forth = (vals[i] & 1) == 0 ? vals[i] : vals[i + 1], back = (vals[i] & 1) == 0 ? vals[i + 1] : vals[i];
      const int sf = forth >> 1, sb = back >> 1;
      c = fv[3 * (size_t)face_of_slot_value(forth, F) + (sf % 3 + 2) % 3];
      d = fv[3 * (size_t)face_of_slot_value(back, F) + (sb % 3 + 2) % 3];
      const bool in_range = (unsigned)c < (unsigned)V && (unsigned)d < (unsigned)V;    // always: included faces
      if (in_range && c != d && !(use_sharp != 0 && edge_sharp(points, fv, vals, i, F, c2))) {
        const int va = valence_of(pairs, n_pairs, a), vb = valence_of(pairs, n_pairs, b);
        const int vc = valence_of(pairs, n_pairs, c), vd = valence_of(pairs, n_pairs, d);
        const int la = lock[a], lb = lock[b], lc = lock[c], ld = lock[d];
        const int before = (deviation(va, la) + deviation(vb, lb)) + (deviation(vc, lc) + deviation(vd, ld));
        const int after = (deviation(va - 1, la) + deviation(vb - 1, lb)) + (deviation(vc + 1, lc) + deviation(vd + 1, ld));
        const int gain = before - after;
        candidate = gain > 0;
        if (candidate) {
          valid = va >= 4 && vb >= 4;
          if (valid) {
            const uint64_t diagonal = edge_key(c, d);
            const int at = lower_bound(pairs, n_pairs, diagonal);
            if (at < n_pairs && pairs[at] == diagonal) valid = false;
          }
          if (valid) {
            const P3 pa = point_of(points, a), pb = point_of(points, b), pc = point_of(points, c), pd = point_of(points, d);
            P3 n0, n1, m0, m1;
            normal_of(pa, pb, pc, n0);
            normal_of(pb, pa, pd, n1);
            normal_of(pa, pd, pc, m0);
            normal_of(pb, pc, pd, m1);
            valid = dot_of(n0, m0) > 0.0 && dot_of(n0, m1) > 0.0 && dot_of(n1, m0) > 0.0 && dot_of(n1, m1) > 0.0 &&
                    dot_of(m0, m1) > 0.0;
          }
          if (valid) key = (uint64_t)(16 - gain) << 32 | (uint64_t)(uint32_t)((keys[i] * 0x9E3779B97F4A7C15ull) >> 32);
        }
      }
    }
    key_out[i] = key;
    idx[i] = i;
    qc[i] = c;
    qd[i] = d;
  }
  count_lanes(candidate, counts + kFlipCandidates);
  count_lanes(valid, counts + kFlipValid);
}

// ---- selection (mesh_select.h): the footprint of a flip is its quad (a, b, c, d), every vertex below V; a selected flip
// notes its position at its two faces
struct FlipQuad {
  static constexpr int kSize = 4;
  const uint64_t* keys;
  const int *vals, *qc, *qd;
  int F, V;
  int* fedge;
  __device__ void footprint(int i, int* v) const {
    v[0] = edge_key_lo(keys[i]); v[1] = edge_key_hi(keys[i]); v[2] = index_from_key(qc[i]); v[3] = index_from_key(qd[i]);
    for (int k = 0; k < 4; ++k)
      if ((unsigned)v[k] >= (unsigned)V) v[k] = 0;                 // never: a live candidate passed the range test
  }
  __device__ void record(int i) const {
    fedge[face_of_slot_value(vals[i], F)] = i;
    fedge[face_of_slot_value(vals[i + 1], F)] = i;
  }
};

__global__ void flip_totals_kernel(int* __restrict__ counts) {
  int flips = 0, sweeps = 0;
  for (int s = 0; s < GEOBI_FLIP_SWEEPS; ++s) {
    flips += counts[kSweepBase + s];
    sweeps += counts[kSweepBase + s] > 0 ? 1 : 0;
  }
  counts[kFlips] = flips;
  counts[kFlipSweeps] = sweeps;
}

// one lane per face: the rows of the two claimants of a selected edge become (a, d, c) and (b, c, d), every other row is
// copied
__global__ void flip_faces_kernel(const int* __restrict__ fv, int F, const uint64_t* __restrict__ keys,
                                  const int* __restrict__ vals, const int* __restrict__ qc, const int* __restrict__ qd,
                                  int n, const int* __restrict__ fedge, int* __restrict__ faces_out) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  int row[3] = {fv[3 * (size_t)f], fv[3 * (size_t)f + 1], fv[3 * (size_t)f + 2]};
  const int i = fedge[f];
  if (i >= 0 && i + 1 < n) {
    const int a = edge_key_lo(keys[i]), b = edge_key_hi(keys[i]), c = qc[i], d = qd[i];
    const int forth = (vals[i] & 1) == 0 ? vals[i] : vals[i + 1];
    if (f == face_of_slot_value(forth, F)) { row[0] = a; row[1] = d; row[2] = c; }
    else { row[0] = b; row[1] = c; row[2] = d; }
  }
  for (int k = 0; k < 3; ++k) faces_out[3 * (size_t)f + k] = row[k];
}

// ---- relaxation
__device__ __forceinline__ void copy_point(const float* __restrict__ from, float* __restrict__ to, int v) {
  for (int k = 0; k < 3; ++k) to[3 * (size_t)v + k] = from[3 * (size_t)v + k];
}

// the proposals of a free vertex v, each from the old positions: -> whether there is one, and `to`
// geobi_relax: towards the mean of the neighbours inside the tangent plane (none for valence < 3 or a normal sum of zero)
struct TangentialProposal {
  double lambda;
  __device__ bool operator()(const float* __restrict__ points, const int* __restrict__ fv, const uint64_t* __restrict__ corners,
                             int n, const uint64_t* __restrict__ pairs, int n_pairs, int v, float* to) const {
#pragma clang fp contract(off)
    double gx = 0.0, gy = 0.0, gz = 0.0;
    int valence = 0;
    for (int j = lower_bound(pairs, n_pairs, (uint64_t)v << 24); j < n_pairs && owner_of(pairs[j]) == v; ++j) {
      const P3 w = point_of(points, item_of(pairs[j]));
      gx = gx + w.x; gy = gy + w.y; gz = gz + w.z;
      ++valence;
    }
    P3 nrm = {0.0, 0.0, 0.0};
    for (int j = lower_bound(corners, n, (uint64_t)v << 24); j < n && owner_of(corners[j]) == v; ++j) {
      P3 nf;
      face_normal(points, fv, item_of(corners[j]), nf);
      nrm.x = nrm.x + nf.x; nrm.y = nrm.y + nf.y; nrm.z = nrm.z + nf.z;
    }
    const double s = dot_of(nrm, nrm);
    if (valence < 3 || s == 0.0) return false;
    const P3 p = point_of(points, v);
    const double count = (double)valence;
    const P3 d = {__ddiv_rn(gx, count) - p.x, __ddiv_rn(gy, count) - p.y, __ddiv_rn(gz, count) - p.z};
    const double q = __ddiv_rn(dot_of(nrm, d), s);
    to[0] = (float)(p.x + lambda * (d.x - nrm.x * q));
    to[1] = (float)(p.y + lambda * (d.y - nrm.y * q));
    to[2] = (float)(p.z + lambda * (d.z - nrm.z * q));
    return true;
  }
};

// geobi_move_to: the given position (none for valence < 3)
struct TargetProposal {
  const float* target;
  __device__ bool operator()(const float* __restrict__, const int* __restrict__, const uint64_t* __restrict__, int,
                             const uint64_t* __restrict__ pairs, int n_pairs, int v, float* to) const {
    if (valence_of(pairs, n_pairs, v) < 3) return false;
    for (int k = 0; k < 3; ++k) to[k] = target[3 * (size_t)v + k];
    return true;
  }
};

// one lane per vertex: the proposal from the old positions, the refusal test against the old positions
template <typename Proposal>
__global__ void relax_move_kernel(const float* __restrict__ points, const int* __restrict__ fv, int V,
                                  const uint64_t* __restrict__ corners, int n, const uint64_t* __restrict__ pairs,
                                  int n_pairs, const int* __restrict__ lock, Proposal proposal, float* __restrict__ out,
                                  int* __restrict__ moved, int* __restrict__ counts) {
#pragma clang fp contract(off)
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  bool moves = false, refused = false;
  if (v < V) {
    float now[3] = {points[3 * (size_t)v], points[3 * (size_t)v + 1], points[3 * (size_t)v + 2]};
    float to[3];
    if (lock[v] == 0 && proposal(points, fv, corners, n, pairs, n_pairs, v, to)) {
      if (!(isfinite(to[0]) && isfinite(to[1]) && isfinite(to[2]))) {
        refused = true;
      } else if (to[0] != now[0] || to[1] != now[1] || to[2] != now[2]) {
        const P3 at = {(double)to[0], (double)to[1], (double)to[2]};
        if (no_flip(points, fv, corners, n, v, -1, at)) {
          moves = true;
          for (int k = 0; k < 3; ++k) now[k] = to[k];
        } else {
          refused = true;
        }
      }
    }
    for (int k = 0; k < 3; ++k) out[3 * (size_t)v + k] = now[k];
    moved[v] = moves ? 1 : 0;
  }
  count_lanes(moves, counts + kMoved);
  count_lanes(refused, counts + kRefused);
}

// one lane per face: an included face with s != 0 whose normal from ALL its new positions turned against the old one is
// counted and (with `revert`) marks its three vertices -- every writer stores the same 1
__global__ void relax_turned_kernel(const float* __restrict__ points, const float* __restrict__ out,
                                    const int* __restrict__ fv, int F, int V, int* __restrict__ revert,
                                    int* __restrict__ counter) {
#pragma clang fp contract(off)
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  bool turned = false;
  if (f < F) {
    int c[3];
    if (face_included(fv, nullptr, f, V, c[0], c[1], c[2])) {
      P3 was, now;
      if (face_normal(points, fv, f, was) != 0.0) {
        face_normal(out, fv, f, now);
        turned = !(dot_of(was, now) > 0.0);
        if (turned && revert != nullptr)
          for (int k = 0; k < 3; ++k) revert[c[k]] = 1;
      }
    }
  }
  if (counter != nullptr) count_lanes(turned, counter);
}

__global__ void relax_revert_kernel(const float* __restrict__ points, int V, const int* __restrict__ moved,
                                    const int* __restrict__ revert, float* __restrict__ out, int* __restrict__ counts) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const bool back = v < V && moved[v] != 0 && revert[v] != 0;
  if (back) copy_point(points, out, v);
  count_lanes(back, counts + kReverted);
}

// ---- statistics: the fp64 length of every edge at the position of its head (-1 elsewhere), the valence of every vertex
__global__ void remesh_lengths_kernel(const uint64_t* __restrict__ keys, int n, const float* __restrict__ points,
                                      double* __restrict__ edge_len) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double len = -1.0;
  if (run_at(keys, n, i).head) {
    len = __dsqrt_rn(edge_len2(points, edge_key_lo(keys[i]), edge_key_hi(keys[i])));
  }
  edge_len[i] = len;
}

__global__ void remesh_valence_kernel(const uint64_t* __restrict__ pairs, int n_pairs, int V, int* __restrict__ valence) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < V) valence[v] = valence_of(pairs, n_pairs, v);
}

struct RemeshBuffers {
  int* counts;
  MeshTables t;                    // the three tables
  // per vertex
  int *m1, *m2, *blocked, *moved, *revert;
  // per sorted position
  uint64_t *key_in, *key_out;
  int *idx_in, *order, *rank, *state, *qc, *qd;
  // per face
  int* fedge;
  PairSort<uint64_t, int> rank_sort;
};
RemeshBuffers carve_remesh(Arena& a, int64_t F, int64_t V) {
  const int64_t n = 3 * F;
  return {a.take<int>(kDevCounts),
          carve_tables<true, true>(a, F),
          a.take<int>(V), a.take<int>(V), a.take<int>(V), a.take<int>(V), a.take<int>(V),
          a.take<uint64_t>(n), a.take<uint64_t>(n),
          a.take<int>(n), a.take<int>(n), a.take<int>(n), a.take<int>(n), a.take<int>(n), a.take<int>(n),
          a.take<int>(F),
          PairSort<uint64_t, int>::take(a, n, 64)};
}

int remesh_buffers(const char* what, int64_t F, int64_t V, void* ws, size_t ws_bytes, RemeshBuffers& b) {
  return carve_checked(what, ws, ws_bytes, b, [&](Arena& a) { return carve_remesh(a, F, V); });
}

// the sorted edge slots, the sorted directed pairs and (with_corners) the sorted corner keys of F > 0 faces; the edge count
// goes to b.counts[edge_count_at]
int build_tables(const RemeshBuffers& b, const int32_t* faces, int64_t F, int64_t V, bool with_corners, int edge_count_at,
                 hipStream_t s) {
  GEOBI_HIP(hipMemsetAsync(b.counts, 0, sizeof(int) * kDevCounts, s));
  GEOBI_TRY(build_edge_table(b.t, faces, nullptr, F, V, s));
  GEOBI_TRY(build_pair_table(b.t, F, nullptr, b.counts + edge_count_at, s));
  if (with_corners) GEOBI_TRY(build_corner_table(b.t, faces, F, V, nullptr, nullptr, s));
  return 0;
}

// the protocol geobi_relax and geobi_move_to share: one lane per vertex proposes and tests, turned / revert / turned
template <typename Proposal>
int guarded_move(const char* what, const int32_t* faces, const float* points, const int32_t* lock, int64_t F, int64_t V,
                 const Proposal& proposal, float* points_out, int32_t* counts, float* stage_ms, void* ws, size_t ws_bytes,
                 hipStream_t s) {
  if (F == 0 || V == 0) {
    GEOBI_HIP(hipMemsetAsync(counts, 0, sizeof(int) * kRelaxCounts, s));
    if (V > 0) GEOBI_HIP(hipMemcpyAsync(points_out, points, sizeof(float) * 3 * (size_t)V, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  RemeshBuffers b;
  GEOBI_TRY(remesh_buffers(what, F, V, ws, ws_bytes, b));
  const int n = (int)(3 * F), n_pairs = 2 * n;
  StageTimer timer(stage_ms, s);
  GEOBI_TRY(timer.mark());
  GEOBI_TRY(build_tables(b, faces, F, V, true, kSpareCount, s));
  GEOBI_HIP(hipMemsetAsync(b.revert, 0, sizeof(int) * (size_t)V, s));
  GEOBI_TRY(timer.mark());
  relax_move_kernel<<<cdiv(V, kT), kT, 0, s>>>(points, faces, (int)V, b.t.c_out, n, b.t.p_out, n_pairs, lock, proposal, points_out,
                                              b.moved, b.counts);
  GEOBI_LAUNCH_OK();
  relax_turned_kernel<<<cdiv(F, kT), kT, 0, s>>>(points, points_out, faces, (int)F, (int)V, b.revert, nullptr);
  GEOBI_LAUNCH_OK();
  relax_revert_kernel<<<cdiv(V, kT), kT, 0, s>>>(points, (int)V, b.moved, b.revert, points_out, b.counts);
  GEOBI_LAUNCH_OK();
  relax_turned_kernel<<<cdiv(F, kT), kT, 0, s>>>(points, points_out, faces, (int)F, (int)V, nullptr, b.counts + kTurned);
  GEOBI_LAUNCH_OK();
  GEOBI_HIP(hipMemcpyAsync(counts, b.counts, sizeof(int) * kRelaxCounts, hipMemcpyDeviceToDevice, s));
  GEOBI_TRY(timer.mark());
  return timer.finish();
}

}  // namespace

}  // namespace geobi

using namespace geobi;

extern "C" {

size_t geobi_remesh_ws_bytes(int64_t F, int64_t V) {
  if (sizes_ok("geobi_remesh_ws_bytes", F > V ? F : V, 0) != 0 || (F < V ? F : V) < 0) return 0;
  return carve_bytes([&](Arena& a) { carve_remesh(a, F, V); });
}

int geobi_remesh_lock(const int32_t* faces, const float* points, int64_t F, int64_t V, int use_sharp, double c2,
                      int32_t* lock, int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(points); GEOBI_NOTNULL(lock); GEOBI_NOTNULL(counts);
  GEOBI_REQUIRE(use_sharp == 0 || (c2 >= 0.0 && c2 <= 1.0), "remesh_lock: c2 = %g (a squared cosine)", c2);
  hipStream_t s = as_stream(stream);
  GEOBI_HIP(hipMemsetAsync(counts, 0, sizeof(int) * kLockCounts, s));
  if (V > 0) GEOBI_HIP(hipMemsetAsync(lock, 0, sizeof(int) * (size_t)V, s));
  if (F == 0 || V == 0) return 0;
  RemeshBuffers b;
  GEOBI_TRY(remesh_buffers("remesh_lock", F, V, ws, ws_bytes, b));
  const int n = (int)(3 * F);
  GEOBI_TRY(build_tables(b, faces, F, V, false, 0, s));
  remesh_lock_kernel<<<cdiv(n, kT), kT, 0, s>>>(b.t.k_out, b.t.v_out, n, points, faces, (int)F, use_sharp, c2, lock, b.counts);
  GEOBI_LAUNCH_OK();
  remesh_lock_counts_kernel<<<cdiv(V, kT), kT, 0, s>>>(lock, (int)V, b.counts);
  GEOBI_LAUNCH_OK();
  GEOBI_HIP(hipMemcpyAsync(counts, b.counts, sizeof(int) * kLockCounts, hipMemcpyDeviceToDevice, s));
  return 0;
}

int geobi_flip_plan(const int32_t* faces, const float* points, const int32_t* lock, int64_t F, int64_t V, int use_sharp,
                    double c2, int32_t* counts, float* stage_ms, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(points); GEOBI_NOTNULL(lock); GEOBI_NOTNULL(counts);
  GEOBI_REQUIRE(use_sharp == 0 || (c2 >= 0.0 && c2 <= 1.0), "flip_plan: c2 = %g (a squared cosine)", c2);
  hipStream_t s = as_stream(stream);
  if (F == 0 || V == 0) {
    GEOBI_HIP(hipMemsetAsync(counts, 0, sizeof(int) * kFlipCounts, s));
    return 0;
  }
  RemeshBuffers b;
  GEOBI_TRY(remesh_buffers("flip_plan", F, V, ws, ws_bytes, b));
  const int n = (int)(3 * F), n_pairs = 2 * n;
  StageTimer timer(stage_ms, s);
  GEOBI_TRY(timer.mark());
  GEOBI_TRY(build_tables(b, faces, F, V, false, 0, s));
  GEOBI_HIP(hipMemsetAsync(b.blocked, 0, sizeof(int) * (size_t)V, s));
  GEOBI_HIP(hipMemsetAsync(b.fedge, 0xff, sizeof(int) * (size_t)F, s));
  GEOBI_TRY(timer.mark());
  // ---- candidates and rank
  flip_candidates_kernel<<<cdiv(n, kT), kT, 0, s>>>(b.t.k_out, b.t.v_out, n, points, faces, (int)F, (int)V, b.t.p_out, n_pairs,
                                                   lock, use_sharp, c2, b.key_in, b.idx_in, b.qc, b.qd, b.counts);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(b.rank_sort.run(b.key_in, b.key_out, b.idx_in, b.order, s));
  rank_kernel<<<cdiv(n, kT), kT, 0, s>>>(b.key_out, b.order, n, b.rank, b.state);
  GEOBI_LAUNCH_OK();
  GEOBI_TRY(timer.mark());
  // ---- selection
  GEOBI_TRY(run_select_sweeps(FlipQuad{b.t.k_out, b.t.v_out, b.qc, b.qd, (int)F, (int)V, b.fedge}, GEOBI_FLIP_SWEEPS, n, V,
                              b.t.p_out, n_pairs, b.rank, b.state, b.m1, b.m2, b.blocked, b.counts + kSweepBase, s));
  flip_totals_kernel<<<1, 1, 0, s>>>(b.counts);
  GEOBI_LAUNCH_OK();
  GEOBI_HIP(hipMemcpyAsync(counts, b.counts, sizeof(int) * kFlipCounts, hipMemcpyDeviceToDevice, s));
  GEOBI_TRY(timer.mark());
  return timer.finish();
}

int geobi_flip_emit(const int32_t* faces, int64_t F, int64_t V, int32_t* faces_out, const void* ws, size_t ws_bytes,
                    void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(faces_out);
  if (F == 0) return 0;
  hipStream_t s = as_stream(stream);
  if (V == 0) {                                      // no plan was made: every row is copied
    GEOBI_HIP(hipMemcpyAsync(faces_out, faces, sizeof(int) * 3 * (size_t)F, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  RemeshBuffers b;
  GEOBI_TRY(remesh_buffers("flip_emit", F, V, const_cast<void*>(ws), ws_bytes, b));
  flip_faces_kernel<<<cdiv(F, kT), kT, 0, s>>>(faces, (int)F, b.t.k_out, b.t.v_out, b.qc, b.qd, (int)(3 * F), b.fedge, faces_out);
  GEOBI_LAUNCH_OK();
  return 0;
}

int geobi_relax(const int32_t* faces, const float* points, const int32_t* lock, int64_t F, int64_t V, double lambda,
                float* points_out, int32_t* counts, float* stage_ms, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(points); GEOBI_NOTNULL(lock); GEOBI_NOTNULL(points_out); GEOBI_NOTNULL(counts);
  GEOBI_REQUIRE(lambda >= 0.0 && lambda <= 1.0, "relax: lambda = %g (in [0, 1])", lambda);
  return guarded_move("relax", faces, points, lock, F, V, TangentialProposal{lambda}, points_out, counts, stage_ms, ws, ws_bytes,
                      as_stream(stream));
}

int geobi_move_to(const int32_t* faces, const float* points, const float* target, const int32_t* lock, int64_t F, int64_t V,
                  float* points_out, int32_t* counts, float* stage_ms, void* ws, size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(points); GEOBI_NOTNULL(target); GEOBI_NOTNULL(lock); GEOBI_NOTNULL(points_out);
  GEOBI_NOTNULL(counts);
  return guarded_move("move_to", faces, points, lock, F, V, TargetProposal{target}, points_out, counts, stage_ms, ws, ws_bytes,
                      as_stream(stream));
}

int geobi_remesh_stats(const int32_t* faces, const float* points, int64_t F, int64_t V, void* edge_len, int32_t* valence,
                       void* ws, size_t ws_bytes, void* stream) {
  GEOBI_MESH_SIZES(F, V);
  GEOBI_NOTNULL(faces); GEOBI_NOTNULL(points); GEOBI_NOTNULL(edge_len); GEOBI_NOTNULL(valence);
  hipStream_t s = as_stream(stream);
  if (V > 0) GEOBI_HIP(hipMemsetAsync(valence, 0, sizeof(int) * (size_t)V, s));
  if (F == 0 || V == 0) return 0;
  RemeshBuffers b;
  GEOBI_TRY(remesh_buffers("remesh_stats", F, V, ws, ws_bytes, b));
  const int n = (int)(3 * F);
  GEOBI_TRY(build_tables(b, faces, F, V, false, 0, s));
  remesh_lengths_kernel<<<cdiv(n, kT), kT, 0, s>>>(b.t.k_out, n, points, (double*)edge_len);
  GEOBI_LAUNCH_OK();
  remesh_valence_kernel<<<cdiv(V, kT), kT, 0, s>>>(b.t.p_out, 2 * n, (int)V, valence);
  GEOBI_LAUNCH_OK();
  return 0;
}

}  // extern "C"
